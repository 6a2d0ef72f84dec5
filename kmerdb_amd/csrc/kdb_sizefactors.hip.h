// kdb_sizefactors.hip.h -- median-of-ratios size factors (Anders & Huber 2010; DESeq2's estimateSizeFactors) and the normalised counts,
// on count vectors where they lie in HBM.  For n vectors x_1 .. x_n of N bins:
//     a bin b is eligible iff x_j[b] > 0 for every j;        L[b] = (1/n) Sum_j ln x_j[b]   (j = 1 .. n in that order, float64)
//     r_j[b] = ln x_j[b] - L[b];     ln s_j = median of r_j over the eligible bins;     normalised count = x_j[b] / s_j
//
// Three kernels, each a grid-stride sweep of chunks of 128 bins per wave, a 16-byte load per lane and vector from a scalar base; the last,
// partial chunk goes through the same loop body with guarded 8-byte accesses, so a bin's arithmetic has one place in the code.
//   geomean_kernel   streams the n vectors once, writes L[b] (nan on ineligible bins: the reserved marker) and counts the eligible bins
//                    exactly: lanes count in 32 bits, waves add by shuffles, one 64-bit integer atomic per wave.
//   select_kernel    one pass of a radix select (kdb_select_host.cpp.h) for every sample at once (blockIdx.y): r_j[b] is recomputed from
//                    x_j[b] and L[b], never stored; among the elements whose key bits above the digit equal the sample's prefix (one or two
//                    prefixes, for the two middle ranks of an even m) the digit is counted into an LDS histogram per workgroup, and the
//                    workgroups' histograms are added into the global one with 64-bit integer atomics.  The digit's position is a runtime
//                    argument: every pass runs this one kernel's code, so the same bin gives the same key bits in every pass.
//   scale_kernel     out[b] = rint(double(x[b]) / s) as uint64, or the quotient itself as float64; out may be x.  A quotient that reaches
//                    2^63 raises a flag word (integer atomic); with `store` off the kernel only looks for one.
// All global accumulation is integer: the same results for any grid and from run to run.  Built without fast-math; the subtraction and the
// division that the contract names are kept from FMA contraction, so that r is the rounded difference of two rounded numbers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kdbhip.h"
#include "kdb_select_host.cpp.h"

namespace kdbsf {

constexpr int TPB = 256;                           // four waves
constexpr int CHUNK_BINS = 128;                    // a wave's step: 64 lanes x 16 bytes
constexpr int WG_BINS = (TPB / 64) * CHUNK_BINS;   // bins one workgroup covers per grid stride
constexpr int MAX_GRID = 1024;                     // workgroups per sample: with 2^36 bins a workgroup meets 2^26, its LDS counters hold 2^32
constexpr uint64_t NBINS_MAX = 1ull << 36;
constexpr int NBUCKET = kdbselect::NBUCKET;
static_assert(WG_BINS == KDB_SIZEFACTORS_WG_BINS && MAX_GRID == KDB_SIZEFACTORS_GRID_MAX, "include/kdbhip.h states the kernels' constants");
static_assert(NBINS_MAX / MAX_GRID < (1ull << 32), "a workgroup's 32-bit histogram counters and a lane's 32-bit eligible count cannot wrap");

typedef unsigned long long u64;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) u64x2 *gvec_t;          // global_load, not flat_load
typedef const __attribute__((address_space(1))) f64x2 *gdvec_t;

struct Target { u64 prefix[2]; uint32_t ntargets, pad; };               // one sample's state of the select (kdbselect::Select)

// bins 2 lane, 2 lane + 1 of chunk `chunk` of vector p: one 16-byte load in a whole chunk, guarded loads (0 past the end) in the last one
__device__ __forceinline__ u64x2 load_bins(const u64 *p, uint64_t chunk, uint32_t lane, uint64_t nbins, bool whole)
{
    if (whole) return ((gvec_t)(p + chunk * CHUNK_BINS))[lane];
    const uint64_t b = chunk * CHUNK_BINS + 2 * lane;
    u64x2 x;
    x.x = b < nbins ? p[b] : 0;
    x.y = b + 1 < nbins ? p[b + 1] : 0;
    return x;
}

__global__ void __launch_bounds__(TPB, 4)
geomean_kernel(const u64 *const *__restrict__ vecs, int n, uint64_t nbins, double *__restrict__ L, u64 *__restrict__ eligible)
{
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nchunks = (nbins + CHUNK_BINS - 1) / CHUNK_BINS;
    const double dn = (double)n;
    uint32_t count = 0;
    for (uint64_t chunk = (uint64_t)blockIdx.x * (TPB / 64) + wave; chunk < nchunks; chunk += (uint64_t)gridDim.x * (TPB / 64)) {
        const bool whole = (chunk + 1) * CHUNK_BINS <= nbins;                          // (wave-uniform)
        double s0 = 0.0, s1 = 0.0;
        bool e0 = true, e1 = true;
        for (int j = 0; j < n; j++) {
            const u64x2 x = load_bins(vecs[j], chunk, lane, nbins, whole);
            e0 = e0 && x.x != 0;
            e1 = e1 && x.y != 0;
            s0 += log((double)x.x);                                                    // (ln 0 = -inf: an ineligible bin's sum is not used)
            s1 += log((double)x.y);
        }
        f64x2 l;
        l.x = e0 ? s0 / dn : __builtin_nan("");
        l.y = e1 ? s1 / dn : __builtin_nan("");
        count += (e0 ? 1u : 0u) + (e1 ? 1u : 0u);
        const uint64_t b = chunk * CHUNK_BINS + 2 * lane;
        if (whole) {
            *(f64x2 *)(L + b) = l;
        } else {
            if (b < nbins) L[b] = l.x;
            if (b + 1 < nbins) L[b + 1] = l.y;
        }
    }
    u64 c = count;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane == 0 && c != 0) atomicAdd(eligible, c);
}

// The key of r = ln x - l: the one place the select's keys come from (geomean_kernel does not share it).
__device__ __forceinline__ uint64_t ratio_key(u64 x, double l)
{
#pragma clang fp contract(off)
    const double r = log((double)x) - l;
    return kdbselect::key_of_bits((uint64_t)__double_as_longlong(r));
}

__device__ __forceinline__ void select_bin(uint32_t (*hist)[NBUCKET], u64 x, double l, u64 p0, u64 p1, bool two, int shift, int width)
{
    if (l != l) return;                                                                // (ineligible, or past the end of the vector)
    const uint64_t key = ratio_key(x, l), above = kdbselect::key_above(key, shift, width);
    const uint32_t digit = kdbselect::key_digit(key, shift, width);
    if (above == p0) atomicAdd(&hist[0][digit], 1u);
    if (two && above == p1) atomicAdd(&hist[1][digit], 1u);
}

// ghist[sample][2][NBUCKET] += this pass's histograms: the digit of `width` bits at `shift`, under targets[sample]'s prefixes
__global__ void __launch_bounds__(TPB, 4)
select_kernel(const u64 *const *__restrict__ vecs, const double *__restrict__ L, uint64_t nbins, const Target *__restrict__ targets, int shift, int width,
              u64 *__restrict__ ghist)
{
    __shared__ uint32_t hist[2][NBUCKET];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Target t = targets[blockIdx.y];
    const bool two = t.ntargets == 2;
    const u64 *px = vecs[blockIdx.y];
    for (int i = threadIdx.x; i < 2 * NBUCKET; i += TPB) (&hist[0][0])[i] = 0;
    __syncthreads();
    const uint64_t nchunks = (nbins + CHUNK_BINS - 1) / CHUNK_BINS;
    for (uint64_t chunk = (uint64_t)blockIdx.x * (TPB / 64) + wave; chunk < nchunks; chunk += (uint64_t)gridDim.x * (TPB / 64)) {
        const bool whole = (chunk + 1) * CHUNK_BINS <= nbins;
        const u64x2 x = load_bins(px, chunk, lane, nbins, whole);
        f64x2 l;
        if (whole) {
            l = ((gdvec_t)(L + chunk * CHUNK_BINS))[lane];
        } else {
            const uint64_t b = chunk * CHUNK_BINS + 2 * lane;
            l.x = b < nbins ? L[b] : __builtin_nan("");
            l.y = b + 1 < nbins ? L[b + 1] : __builtin_nan("");
        }
        select_bin(hist, x.x, l.x, t.prefix[0], t.prefix[1], two, shift, width);
        select_bin(hist, x.y, l.y, t.prefix[0], t.prefix[1], two, shift, width);
    }
    __syncthreads();
    u64 *out = ghist + (uint64_t)blockIdx.y * 2 * NBUCKET;
    for (int i = threadIdx.x; i < (two ? 2 : 1) * NBUCKET; i += TPB) {
        const uint32_t c = (&hist[0][0])[i];
        if (c != 0) atomicAdd(out + i, (u64)c);
    }
}

// out[b] = rint(x[b] / s) as uint64 (as_float64 == 0) or x[b] / s as float64; *flag |= 1 if a rounded quotient reaches 2^63 (integer output
// only).  store == 0: look for such a quotient and write nothing.  x and out may be the same vector: a lane reads its bins before it writes them.
__global__ void __launch_bounds__(TPB, 4)
scale_kernel(const u64 *x, uint64_t nbins, double s, void *out, int as_float64, int store, uint32_t *__restrict__ flag)
{
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nchunks = (nbins + CHUNK_BINS - 1) / CHUNK_BINS;
    bool over = false;
    for (uint64_t chunk = (uint64_t)blockIdx.x * (TPB / 64) + wave; chunk < nchunks; chunk += (uint64_t)gridDim.x * (TPB / 64)) {
        const bool whole = (chunk + 1) * CHUNK_BINS <= nbins;
        const u64x2 v = load_bins(x, chunk, lane, nbins, whole);
        const double q0 = (double)v.x / s, q1 = (double)v.y / s;
        u64x2 w;
        if (as_float64) {
            w.x = (u64)__double_as_longlong(q0);
            w.y = (u64)__double_as_longlong(q1);
        } else {
            const double r0 = rint(q0), r1 = rint(q1);
            const bool o0 = r0 >= 9223372036854775808.0, o1 = r1 >= 9223372036854775808.0;
            over = over || o0 || o1;
            w.x = o0 ? 0 : (u64)r0;
            w.y = o1 ? 0 : (u64)r1;
        }
        if (!store) continue;
        u64 *o = (u64 *)out;
        const uint64_t b = chunk * CHUNK_BINS + 2 * lane;
        if (whole) {
            *(u64x2 *)(o + b) = w;
        } else {
            if (b < nbins) o[b] = w.x;
            if (b + 1 < nbins) o[b + 1] = w.y;
        }
    }
    if (__any(over) && lane == 0) atomicOr(flag, 1u);
}

}  // namespace kdbsf
