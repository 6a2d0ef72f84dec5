// kdb_analysis_host.hip.h -- host side of the analysis calls of include/kdbhip.h, the ones that take finished vectors and no kdb_engine:
// kdb_gram, kdb_pairstats, kdb_pairfloat, kdb_size_factors, kdb_scale_counts, kdb_spectrum, kdb_rank_transform, kdb_strand_merge,
// kdb_score_reads, and kdb_record_tables, kdb_minimizers, kdb_align_banded and kdb_align_traceback (which take residues alone).  Every call works in an AnalysisCall: its own stream, events and
// scratch, gone when it returns.  What the host alone decides -- rows, groups, grids, pieces -- is kdb_sweep_plan.cpp.h's.  The three calls that
// take residues and record offsets (kdb_score_reads, kdb_record_tables, kdb_minimizers) check them with record_check_args / record_check_sizes
// and bring them and their kdbplan::RecordLayout to the device through one RecordBatch; kdb_align_banded and kdb_align_traceback share
// their checks (align_check_scalars, align_check_batch) and stage their word-padded buffers through one AlignBatch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <optional>
#include <vector>

#include "../../include/kdbhip.h"
#include "kdb_hostutil.hip.h"
#include "kdb_kernels.hip.h"
#include "kdb_gram.hip.h"
#include "kdb_pairstats.hip.h"
#include "kdb_sizefactors.hip.h"
#include "kdb_select_host.cpp.h"
#include "kdb_spectrum.hip.h"
#include "kdb_spectrum_host.cpp.h"
#include "kdb_strands.hip.h"
#include "kdb_score.hip.h"
#include "kdb_tables.hip.h"
#include "kdb_minimizers.hip.h"
#include "kdb_align.hip.h"
#include "kdb_align_trace.hip.h"
#include "kdb_sweep_plan.cpp.h"

namespace {

// One analysis call's hold on the device: the checked and selected device, a non-blocking stream, the two events around its kernels (made
// at the first span) and its scratch.
struct AnalysisCall {
    std::optional<DeviceGuard> guard;      // (declared first: the device stays selected while the destructor frees)
    std::vector<void *> allocs;
    hipStream_t st = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    double ms = 0.0;                       // device time of the spans measured so far

    int open(int device_id)
    {
        int ndev = 0;
        HIP_TRY(hipGetDeviceCount(&ndev));
        if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
        guard.emplace(device_id);
        HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return KDB_OK;
    }
    // `count` Ts of device memory, the call's until it ends; null where there is no room (and no HIP error is left behind)
    template <class T>
    T *alloc(uint64_t count)
    {
        void *p = nullptr;
        if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        allocs.push_back(p);
        return (T *)p;
    }
    void release(void *p) { allocs.erase(std::remove(allocs.begin(), allocs.end(), p), allocs.end()); (void)hipFree(p); }
    // begin() ... end(): a span of the stream; elapsed(), once the stream has been synchronised, adds its device time to ms and gives the
    // sum to *out, where the caller asked for the time
    hipError_t begin()
    {
        hipError_t e = hipSuccess;
        if ((!a && (e = hipEventCreate(&a)) != hipSuccess) || (!b && (e = hipEventCreate(&b)) != hipSuccess)) return e;
        return hipEventRecord(a, st);
    }
    hipError_t end() { return hipEventRecord(b, st); }
    hipError_t elapsed(double *out = nullptr)
    {
        float t = 0;
        const hipError_t e = hipEventElapsedTime(&t, a, b);
        ms += (double)t;
        if (out && e == hipSuccess) *out = ms;
        return e;
    }
    ~AnalysisCall()
    {
        for (void *p : allocs) (void)hipFree(p);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        if (st) (void)hipStreamDestroy(st);
    }
};

// the grid of kdb_gram's and kdb_pairstats' sweeps, the caps as include/kdbhip.h states them
kdbplan::Grid gram_grid(uint64_t nbins, uint32_t chunk_bins, uint32_t wg_chunks, uint32_t nrows)
{
    return kdbplan::sweep_grid(nbins, chunk_bins, wg_chunks, kdbplan::rows_cap(nrows, KDB_GRAM_GRID_MANY_ROWS, KDB_GRAM_GRID_MAX, KDB_GRAM_GRID_MAX_MANY_ROWS));
}

// kdb_gram: the launch of one group of rows, by the sizes of its blocks
void gram_launch(const kdbplan::Group &gr, uint32_t gx, const unsigned long long *const *vecs, const kdbgram::Row *rows, uint32_t nchunks, uint32_t pstride, ulonglong2 *partials,
                 hipStream_t st)
{
    const dim3 grid(gx, gr.nrows), block(kdbgram::TPB);
    const kdbgram::Row *r = rows + gr.row0;
    ulonglong2 *p = partials + (uint64_t)gr.row0 * pstride * kdbgram::NSLOT;
#define KDB_GRAM_CASE(NA, NB, DIAG) hipLaunchKernelGGL((kdbgram::gram_kernel<NA, NB, DIAG>), grid, block, 0, st, vecs, r, nchunks, pstride, p)
    if (gr.diag) {
        switch (gr.na) {
            case 1: KDB_GRAM_CASE(1, 1, true); break;
            case 2: KDB_GRAM_CASE(2, 2, true); break;
            case 3: KDB_GRAM_CASE(3, 3, true); break;
            default: KDB_GRAM_CASE(4, 4, true); break;
        }
    } else {                                           // (off the diagonal the first block is always a full one)
        switch (gr.nb) {
            case 1: KDB_GRAM_CASE(4, 1, false); break;
            case 2: KDB_GRAM_CASE(4, 2, false); break;
            case 3: KDB_GRAM_CASE(4, 3, false); break;
            default: KDB_GRAM_CASE(4, 4, false); break;
        }
    }
#undef KDB_GRAM_CASE
}

int pair_check_args(const char *who, const void *const *d_vectors, int n, uint64_t nbins)
{
    if (n < 1 || n > KDB_GRAM_MAX) return fail(KDB_ERR_ARG, "%s: n=%d, 1..%d vectors supported", who, n, KDB_GRAM_MAX);
    if (nbins == 0 || nbins > kdbpair::NBINS_MAX) return fail(KDB_ERR_ARG, "%s: nbins is 0 or above 2^36 (64 x 4^17: more than a device holds)", who);
    if (!d_vectors) return fail(KDB_ERR_ARG, "%s: d_vectors must not be NULL", who);
    for (int i = 0; i < n; i++) {
        if (!d_vectors[i]) return fail(KDB_ERR_ARG, "%s: vector %d is NULL", who, i);
        if (((uintptr_t)d_vectors[i] & 15u) != 0) return fail(KDB_ERR_ARG, "%s: vector %d is not 16-byte aligned", who, i);
    }
    return KDB_OK;
}

void pair_launch(const kdbplan::Group &gr, uint32_t gx, const unsigned long long *const *vecs, const kdbpair::Row *rows, uint32_t nchunks, uint32_t pstride,
                 unsigned long long *partials, hipStream_t st)
{
    const dim3 grid(gx, gr.nrows), block(kdbpair::TPB);
    const kdbpair::Row *r = rows + gr.row0;
    unsigned long long *p = partials + (uint64_t)gr.row0 * pstride * kdbpair::ROW_WORDS;
#define KDB_PAIR_CASE(NA, NB, DIAG) hipLaunchKernelGGL((kdbpair::pair_kernel<NA, NB, DIAG>), grid, block, 0, st, vecs, r, nchunks, pstride, p)
    if (gr.diag) {
        switch (gr.na) {
            case 1: KDB_PAIR_CASE(1, 1, true); break;
            case 2: KDB_PAIR_CASE(2, 2, true); break;
            case 3: KDB_PAIR_CASE(3, 3, true); break;
            default: KDB_PAIR_CASE(4, 4, true); break;
        }
    } else {                                           // (off the diagonal the first block is always a full one)
        if (gr.nb == 1) KDB_PAIR_CASE(4, 1, false);
        else KDB_PAIR_CASE(4, 2, false);
    }
#undef KDB_PAIR_CASE
}

uint32_t sizefactor_grid(uint64_t nbins) { return kdbplan::sweep_grid(nbins, kdbsf::CHUNK_BINS, kdbsf::TPB / 64, kdbsf::MAX_GRID, false).gx; }

// kdb_spectrum, kdb_rank_transform: the table of multiplicities (DENSE words, then the overflow list's counter) and the list of `cap` values
struct SpectrumScratch { unsigned long long *dense = nullptr, *over = nullptr; uint64_t cap = 0; };

// what both entry points check first; nothing on the device is touched
int spectrum_check_args(const char *who, const void *d_vector, uint64_t nbins)
{
    if (!d_vector) return fail(KDB_ERR_ARG, "%s: the vector is NULL", who);
    if (((uintptr_t)d_vector & 15u) != 0) return fail(KDB_ERR_ARG, "%s: the vector is not 16-byte aligned", who);
    if (nbins == 0 || nbins > kdbspectrum::MAX_BINS) return fail(KDB_ERR_ARG, "%s: nbins is 0 or above 2^36 (64 x 4^17: more than a device holds)", who);
    return KDB_OK;
}

// (re)allocate the list for `cap` values; the table at the first call
int spectrum_alloc(const char *who, AnalysisCall &call, SpectrumScratch &sc, uint64_t cap)
{
    if (!sc.dense && !(sc.dense = call.alloc<unsigned long long>(kdbspectrum::DENSE + 1)))
        return fail(KDB_ERR_NOMEM, "%s: no room for the table of %u multiplicities", who, kdbspectrum::DENSE);
    if (sc.over) call.release(sc.over);
    sc.over = nullptr;
    sc.cap = 0;
    if (cap && !(sc.over = call.alloc<unsigned long long>(cap)))
        return fail(KDB_ERR_NOMEM, "%s: no room for a list of %llu values of 65536 and above", who, (unsigned long long)cap);
    sc.cap = cap;
    return KDB_OK;
}

// one sweep: host[0 .. DENSE) = the multiplicities, host[DENSE] = how many values the list would hold (sc.cap of them are stored); call.ms += device time
int spectrum_sweep(AnalysisCall &call, const SpectrumScratch &sc, const void *d_vector, uint64_t nbins, std::vector<uint64_t> &host)
{
    const uint64_t nchunks = nbins / kdbspectrum::CHUNK_BINS;
    host.assign(kdbspectrum::DENSE + 1, 0);
    HIP_TRY(hipMemsetAsync(sc.dense, 0, (kdbspectrum::DENSE + 1) * 8ull, call.st));
    HIP_TRY(call.begin());
    hipLaunchKernelGGL(kdbspectrum::spectrum_kernel, dim3(kdbspectrum::spectrum_grid(nchunks)), dim3(kdbspectrum::TPB), 0, call.st,
                       (const unsigned long long *)d_vector, nbins, nchunks, sc.dense, sc.over, (unsigned long long)sc.cap, sc.dense + kdbspectrum::DENSE);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    HIP_TRY(hipMemcpyAsync(host.data(), sc.dense, (kdbspectrum::DENSE + 1) * 8ull, hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed());
    uint64_t total = host[kdbspectrum::DENSE];
    for (uint32_t v = 0; v < kdbspectrum::DENSE; v++) total += host[v];
    if (total != nbins) return fail(KDB_ERR_HIP, "the spectrum holds %llu bins, the vector %llu", (unsigned long long)total, (unsigned long long)nbins);
    return KDB_OK;
}

// how many of the nbytes residues are not one of upper-case ACGTN
// (a block at a time into one byte, which the compiler keeps in byte lanes: 4-5 x the rate of counting into 64 bits; a block is
// counted only where it holds an offender)
uint64_t residues_outside_acgtn(const uint8_t *bases, size_t nbytes)
{
    uint64_t nbad = 0;
    auto outside = [](uint8_t b) { return !((b == 'A') | (b == 'C') | (b == 'G') | (b == 'T') | (b == 'N')); };
    for (size_t at = 0; at < nbytes; at += 4096) {
        const size_t n = std::min<size_t>(4096, nbytes - at);
        uint8_t any = 0;
        for (size_t i = 0; i < n; i++) any |= (uint8_t)outside(bases[at + i]);
        if (any) for (size_t i = 0; i < n; i++) nbad += outside(bases[at + i]);
    }
    return nbad;
}

// ---- what kdb_score_reads, kdb_record_tables and kdb_minimizers share: nbytes residues, the nreads + 1 offsets of their records ----

// The batch's buffers; outputs: none of the call's own output arrays is NULL.  A batch without records passes: the caller answers it.
int record_check_args(const char *who, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads, bool outputs)
{
    if (nreads == 0) return nbytes == 0 ? KDB_OK : fail(KDB_ERR_ARG, "%s: residues but no records", who);
    if (!offs || (!bases && nbytes) || !outputs) return fail(KDB_ERR_ARG, "%s: NULL buffer", who);
    return KDB_OK;
}

// the sizes the layout counts on: its piece indices then stay below 2^31
int record_check_sizes(const char *who, size_t nbytes, size_t nreads)
{
    if (nbytes > (1ull << 30)) return fail(KDB_ERR_ARG, "%s: at most 2^30 residues per call", who);
    if (nreads > (1ull << 30)) return fail(KDB_ERR_ARG, "%s: at most 2^30 records per call", who);
    return KDB_OK;
}

// the refusal of offsets that kdbplan::check_offsets() did not pass
int record_offsets_fail(kdbplan::LayoutError bad)
{
    return fail(KDB_ERR_ARG, bad == kdbplan::LAYOUT_ENDS ? "read_offsets must start at 0 and end at nbytes" : "read_offsets must rise from 0 to nbytes");
}

// The batch on the device: the residues -- whole 16-byte lines and `pad` bytes more, for the aligned words the kernels read past a window's
// start --, the offsets and the two arrays of the layout; piece_rec stays null where the layout has none.
struct RecordBatch {
    uint8_t *bases = nullptr;
    uint64_t *offs = nullptr;
    uint32_t *rec_piece0 = nullptr, *piece_rec = nullptr;

    // false: no room for one of them
    bool alloc(AnalysisCall &call, size_t nbytes, size_t nreads, const kdbplan::RecordLayout &lay, size_t pad)
    {
        bases = call.alloc<uint8_t>(((nbytes + 15) & ~(size_t)15) + pad);
        offs = call.alloc<uint64_t>(nreads + 1);
        rec_piece0 = call.alloc<uint32_t>(nreads + 1);
        if (!lay.piece_rec.empty()) piece_rec = call.alloc<uint32_t>(lay.npieces);
        return bases && offs && rec_piece0 && (lay.piece_rec.empty() || piece_rec);
    }
    int upload(AnalysisCall &call, const uint8_t *h_bases, size_t nbytes, const uint64_t *h_offs, size_t nreads, const kdbplan::RecordLayout &lay)
    {
        if (nbytes) HIP_TRY(hipMemcpyAsync(bases, h_bases, nbytes, hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(offs, h_offs, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(rec_piece0, lay.rec_piece0.data(), (nreads + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, call.st));
        if (piece_rec) HIP_TRY(hipMemcpyAsync(piece_rec, lay.piece_rec.data(), lay.npieces * sizeof(uint32_t), hipMemcpyHostToDevice, call.st));
        return KDB_OK;
    }
};

}  // namespace

extern "C" {

// ---- exact moments of finished vectors (kdb_gram.hip.h): sums and Gram matrix as 128-bit integers ----
int kdb_gram(int device_id, const void *const *d_vectors, int n, uint64_t nbins, uint64_t *sums_out, uint64_t *gram_out, double *kernel_ms_out)
{
    constexpr int B = kdbgram::B, NSLOT = kdbgram::NSLOT;
    if (n < 1 || n > KDB_GRAM_MAX) return fail(KDB_ERR_ARG, "kdb_gram: n=%d, 1..%d vectors supported", n, KDB_GRAM_MAX);
    if (nbins == 0 || nbins > (1ull << 36)) return fail(KDB_ERR_ARG, "kdb_gram: nbins is 0 or above 2^36 (64 x 4^17: more than a device holds)");
    if (!d_vectors || !sums_out || !gram_out) return fail(KDB_ERR_ARG, "kdb_gram: d_vectors, sums_out and gram_out must not be NULL");
    for (int i = 0; i < n; i++) {
        if (!d_vectors[i]) return fail(KDB_ERR_ARG, "kdb_gram: vector %d is NULL", i);
        if (((uintptr_t)d_vectors[i] & 15u) != 0) return fail(KDB_ERR_ARG, "kdb_gram: vector %d is not 16-byte aligned", i);
    }
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    const kdbplan::Plan<kdbgram::Row> plan = kdbplan::gram_plan<kdbgram::Row>(n, B);
    const std::vector<kdbgram::Row> &rows = plan.rows;
    const uint32_t nrows = (uint32_t)rows.size();
    // gram_kernel takes the whole chunks, gram_tail_kernel the bins behind them; a row's partials: one per workgroup, then the tail's
    const auto [nchunks, gx, nparts] = gram_grid(nbins, kdbgram::CHUNK_BINS, kdbgram::TPB / 64, nrows);                // (any grid gives the same integers)
    std::vector<const unsigned long long *> ptrs((size_t)(n + B - 1) / B * B, (const unsigned long long *)d_vectors[0]);
    for (int i = 0; i < n; i++) ptrs[i] = (const unsigned long long *)d_vectors[i];
    auto *d_vecs = call.alloc<const unsigned long long *>(ptrs.size());
    auto *d_rows = call.alloc<kdbgram::Row>(nrows);
    auto *partials = call.alloc<ulonglong2>((uint64_t)nrows * nparts * NSLOT), *out = call.alloc<ulonglong2>((uint64_t)nrows * NSLOT);
    if (!d_vecs || !d_rows || !partials || !out) return fail(KDB_ERR_NOMEM, "kdb_gram: no room for the partial sums of %u x %u workgroups", nrows, gx);
    HIP_TRY(hipMemcpyAsync(d_vecs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), nrows * sizeof(kdbgram::Row), hipMemcpyHostToDevice, call.st));
    HIP_TRY(call.begin());
    for (const kdbplan::Group &gr : plan.groups) gram_launch(gr, gx, d_vecs, d_rows, nchunks, nparts, partials, call.st);
    hipLaunchKernelGGL(kdbgram::gram_tail_kernel, dim3(nrows), dim3(64), 0, call.st, d_vecs, (const kdbgram::Row *)d_rows, n, (uint64_t)nchunks * kdbgram::CHUNK_BINS, nbins,
                       nparts, gx, partials);
    hipLaunchKernelGGL(kdbgram::gram_combine_kernel, dim3(nrows), dim3(256), 0, call.st, (const ulonglong2 *)partials, nparts, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    std::vector<ulonglong2> res((size_t)nrows * NSLOT);
    HIP_TRY(hipMemcpyAsync(res.data(), out, res.size() * sizeof(ulonglong2), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    for (uint32_t r = 0; r < nrows; r++) {
        const ulonglong2 *slot = &res[(size_t)r * NSLOT];
        for (int i = 0; i < B; i++) {
            const int vi = rows[r].bi * B + i;
            if (vi >= n) continue;
            if (rows[r].bi == rows[r].bj) { sums_out[2 * vi] = slot[B * B + i].x; sums_out[2 * vi + 1] = slot[B * B + i].y; }
            for (int j = 0; j < B; j++) {
                const int vj = rows[r].bj * B + j;
                if (vj >= n || vj < vi) continue;
                const ulonglong2 v = slot[i * B + j];
                gram_out[2 * ((size_t)vi * n + vj)] = gram_out[2 * ((size_t)vj * n + vi)] = v.x;
                gram_out[2 * ((size_t)vi * n + vj) + 1] = gram_out[2 * ((size_t)vj * n + vi) + 1] = v.y;
            }
        }
    }
    for (int i = 0; i < n; i++)
        if (sums_out[2 * i + 1] != 0)
            return fail(KDB_ERR_ARG, "kdb_gram: the sum of vector %d is 2^64 or more: its products may have wrapped 128 bits", i);
    return KDB_OK;
}

// ---- the pairwise statistics that are not moments (kdb_pairstats.hip.h): exact integers, and the float sweep of canberra / jensenshannon ----
int kdb_pairstats(int device_id, const void *const *d_vectors, int n, uint64_t nbins, uint64_t *sums_out, uint64_t *nnz_out, uint64_t *l1_out,
                  uint64_t *linf_out, uint64_t *ne_out, uint64_t *both_out, double *kernel_ms_out)
{
    constexpr int B = kdbpair::B, NPAIR = kdbpair::NPAIR, PW = kdbpair::PAIR_WORDS, VW = kdbpair::VEC_WORDS, RW = kdbpair::ROW_WORDS;
    if (int rc = pair_check_args("kdb_pairstats", d_vectors, n, nbins)) return rc;
    if (!sums_out || !nnz_out || !l1_out || !linf_out || !ne_out || !both_out) return fail(KDB_ERR_ARG, "kdb_pairstats: the six output arrays must not be NULL");
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    const kdbplan::Plan<kdbpair::Row> plan = kdbplan::pair_plan<kdbpair::Row>(n, B, kdbpair::HALF);
    const std::vector<kdbpair::Row> &rows = plan.rows;
    const uint32_t nrows = (uint32_t)rows.size();
    // pair_kernel takes the whole chunks, pair_tail_kernel the bins behind them; a row's partials: one per workgroup, then the tail's
    const auto [nchunks, gx, nparts] = gram_grid(nbins, kdbpair::CHUNK_BINS, kdbpair::TPB / 64, nrows);                // (any grid gives the same integers)
    std::vector<const unsigned long long *> ptrs((size_t)n);
    for (int i = 0; i < n; i++) ptrs[i] = (const unsigned long long *)d_vectors[i];
    auto *d_vecs = call.alloc<const unsigned long long *>(ptrs.size());
    auto *d_rows = call.alloc<kdbpair::Row>(nrows);
    auto *partials = call.alloc<unsigned long long>((uint64_t)nrows * nparts * RW), *out = call.alloc<unsigned long long>((uint64_t)nrows * RW);
    if (!d_vecs || !d_rows || !partials || !out) return fail(KDB_ERR_NOMEM, "kdb_pairstats: no room for the partial records of %u x %u workgroups", nrows, gx);
    HIP_TRY(hipMemcpyAsync(d_vecs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), nrows * sizeof(kdbpair::Row), hipMemcpyHostToDevice, call.st));
    HIP_TRY(call.begin());
    for (const kdbplan::Group &gr : plan.groups) pair_launch(gr, gx, d_vecs, d_rows, nchunks, nparts, partials, call.st);
    hipLaunchKernelGGL(kdbpair::pair_tail_kernel, dim3(nrows), dim3(64), 0, call.st, d_vecs, (const kdbpair::Row *)d_rows, (uint64_t)nchunks * kdbpair::CHUNK_BINS, nbins,
                       nparts, gx, partials);
    hipLaunchKernelGGL(kdbpair::pair_combine_kernel, dim3(nrows), dim3(256), 0, call.st, (const unsigned long long *)partials, nparts, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    std::vector<unsigned long long> res((size_t)nrows * RW);
    HIP_TRY(hipMemcpyAsync(res.data(), out, res.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    for (uint32_t r = 0; r < nrows; r++) {
        const unsigned long long *rec = &res[(size_t)r * RW];
        const kdbpair::Row &row = rows[r];
        const bool diag = row.a0 == row.b0;
        for (int i = 0; i < row.na; i++) {
            const size_t vi = (size_t)row.a0 + i;
            if (diag) {
                const unsigned long long *v = rec + NPAIR * PW + i * VW;
                sums_out[2 * vi] = v[0]; sums_out[2 * vi + 1] = v[1]; nnz_out[vi] = v[2];
                l1_out[2 * (vi * n + vi)] = l1_out[2 * (vi * n + vi) + 1] = linf_out[vi * n + vi] = ne_out[vi * n + vi] = 0;
                both_out[vi * n + vi] = v[2];
            }
            for (int j = diag ? i + 1 : 0; j < row.nb; j++) {
                const size_t vj = (size_t)row.b0 + j, at = vi * n + vj, ta = vj * n + vi;
                const unsigned long long *p = rec + (i * B + j) * PW;
                l1_out[2 * at] = l1_out[2 * ta] = p[0];
                l1_out[2 * at + 1] = l1_out[2 * ta + 1] = p[1];
                linf_out[at] = linf_out[ta] = p[2];
                ne_out[at] = ne_out[ta] = p[3];
                both_out[at] = both_out[ta] = p[4];
            }
        }
    }
    for (int i = 0; i < n; i++)
        if (sums_out[2 * i + 1] != 0)
            return fail(KDB_ERR_ARG, "kdb_pairstats: the sum of vector %d is 2^64 or more: L1 of a pair with it may not fit its two words", i);
    return KDB_OK;
}

int kdb_pairfloat(int device_id, const void *const *d_vectors, int n, uint64_t nbins, double *canberra_out, double *js_out, double *kernel_ms_out)
{
    constexpr int FW = kdbpair::FLOAT_WORDS;
    if (int rc = pair_check_args("kdb_pairfloat", d_vectors, n, nbins)) return rc;
    if (!canberra_out || !js_out) return fail(KDB_ERR_ARG, "kdb_pairfloat: canberra_out and js_out must not be NULL");
    // the exact sums (and the refusal of one that reaches 2^64), from the integer sweep
    const size_t nn = (size_t)n * n;
    std::vector<uint64_t> isums(2 * (size_t)n), scratch64(6 * nn + n);
    if (int rc = kdb_pairstats(device_id, d_vectors, n, nbins, isums.data(), scratch64.data() + 6 * nn, scratch64.data(), scratch64.data() + 2 * nn,
                               scratch64.data() + 3 * nn, scratch64.data() + 4 * nn, nullptr))
        return rc;
    std::vector<double> sums((size_t)n);
    for (int i = 0; i < n; i++) sums[i] = (double)isums[2 * i];                       // (one rounding; the high word is zero)
    for (size_t i = 0; i < nn; i++) canberra_out[i] = js_out[i] = 0.0;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (n < 2) return KDB_OK;
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    const std::vector<kdbpair::FloatRow> rows = kdbplan::float_rows<kdbpair::FloatRow>(n);
    const uint32_t nrows = (uint32_t)rows.size();
    const auto [nchunks, gx, nparts] = kdbplan::sweep_grid(nbins, kdbpair::CHUNK_BINS, kdbpair::TPB / 64, KDB_PAIRFLOAT_GRID_MAX);      // (a function of nbins alone: the order of the additions is fixed)
    std::vector<const unsigned long long *> ptrs((size_t)n);
    for (int i = 0; i < n; i++) ptrs[i] = (const unsigned long long *)d_vectors[i];
    auto *d_vecs = call.alloc<const unsigned long long *>(ptrs.size());
    auto *d_rows = call.alloc<kdbpair::FloatRow>(nrows);
    auto *d_sums = call.alloc<double>(sums.size()), *partials = call.alloc<double>((uint64_t)nrows * nparts * FW), *out = call.alloc<double>((uint64_t)nrows * FW);
    if (!d_vecs || !d_rows || !d_sums || !partials || !out) return fail(KDB_ERR_NOMEM, "kdb_pairfloat: no room for the partial sums of %u x %u workgroups", nrows, gx);
    HIP_TRY(hipMemcpyAsync(d_vecs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), nrows * sizeof(kdbpair::FloatRow), hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipMemcpyAsync(d_sums, sums.data(), sums.size() * sizeof(double), hipMemcpyHostToDevice, call.st));
    HIP_TRY(call.begin());
    hipLaunchKernelGGL(kdbpair::pairfloat_kernel, dim3(gx, nrows), dim3(kdbpair::TPB), 0, call.st, d_vecs, (const kdbpair::FloatRow *)d_rows, (const double *)d_sums, nchunks,
                       nparts, partials);
    hipLaunchKernelGGL(kdbpair::pairfloat_tail_kernel, dim3(nrows), dim3(64), 0, call.st, d_vecs, (const kdbpair::FloatRow *)d_rows, (const double *)d_sums,
                       (uint64_t)nchunks * kdbpair::CHUNK_BINS, nbins, nparts, gx, partials);
    hipLaunchKernelGGL(kdbpair::pairfloat_combine_kernel, dim3(nrows), dim3(64), 0, call.st, (const double *)partials, nparts, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    std::vector<double> res((size_t)nrows * FW);
    HIP_TRY(hipMemcpyAsync(res.data(), out, res.size() * sizeof(double), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    for (uint32_t r = 0; r < nrows; r++) {
        const size_t i = rows[r].i, j = rows[r].j;
        const bool empty = isums[2 * i] == 0 || isums[2 * j] == 0;
        canberra_out[i * n + j] = canberra_out[j * n + i] = res[(size_t)r * FW];
        js_out[i * n + j] = js_out[j * n + i] = empty ? (double)NAN : res[(size_t)r * FW + 1];
    }
    return KDB_OK;
}

// ---- median-of-ratios size factors and normalised counts (kdb_sizefactors.hip.h, kdb_select_host.cpp.h) ----
int kdb_size_factors(int device_id, const void *const *d_vectors, int n, uint64_t nbins, double *log_sf_out, uint64_t *eligible_out, double *kernel_ms_out)
{
    constexpr int NB = kdbsf::NBUCKET;
    if (int rc = pair_check_args("kdb_size_factors", d_vectors, n, nbins)) return rc;
    if (!log_sf_out || !eligible_out) return fail(KDB_ERR_ARG, "kdb_size_factors: log_sf_out and eligible_out must not be NULL");
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    std::vector<const unsigned long long *> ptrs((size_t)n);
    for (int i = 0; i < n; i++) ptrs[i] = (const unsigned long long *)d_vectors[i];
    const size_t hist_bytes = (size_t)n * 2 * NB * sizeof(uint64_t);
    auto *L = call.alloc<double>((nbins + 1) & ~1ull);
    auto *d_vecs = call.alloc<const unsigned long long *>(ptrs.size());
    auto *d_eligible = call.alloc<unsigned long long>(1), *d_hist = call.alloc<unsigned long long>((size_t)n * 2 * NB);
    auto *d_targets = call.alloc<kdbsf::Target>((size_t)n);
    if (!L || !d_vecs || !d_eligible || !d_hist || !d_targets)
        return fail(KDB_ERR_NOMEM, "kdb_size_factors: no room for the float64 scratch of %llu bins", (unsigned long long)nbins);
    const uint32_t gx = sizefactor_grid(nbins);                                        // (any grid gives the same integers)

    uint64_t m = 0;
    HIP_TRY(hipMemcpyAsync(d_vecs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipMemsetAsync(d_eligible, 0, sizeof(uint64_t), call.st));
    HIP_TRY(call.begin());
    hipLaunchKernelGGL(kdbsf::geomean_kernel, dim3(gx), dim3(kdbsf::TPB), 0, call.st, d_vecs, n, nbins, L, d_eligible);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    HIP_TRY(hipMemcpyAsync(&m, d_eligible, sizeof(uint64_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed());
    *eligible_out = m;
    if (kernel_ms_out) *kernel_ms_out = call.ms;
    if (m == 0) {
        for (int j = 0; j < n; j++) log_sf_out[j] = (double)NAN;
        return KDB_OK;
    }

    std::vector<kdbselect::Select> sel((size_t)n);
    uint64_t lo, hi;
    kdbselect::median_ranks(m, &lo, &hi);
    for (auto &s : sel) s.start(lo, hi);
    std::vector<kdbsf::Target> targets((size_t)n);
    std::vector<uint64_t> hist((size_t)n * 2 * NB);
    for (int pass = 0; pass < kdbselect::NPASS; pass++) {
        for (int j = 0; j < n; j++) targets[j] = kdbsf::Target{{sel[j].prefix[0], sel[j].prefix[1]}, (uint32_t)sel[j].ntargets, 0};
        HIP_TRY(hipMemcpyAsync(d_targets, targets.data(), targets.size() * sizeof(kdbsf::Target), hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemsetAsync(d_hist, 0, hist_bytes, call.st));
        HIP_TRY(call.begin());
        hipLaunchKernelGGL(kdbsf::select_kernel, dim3(gx, (uint32_t)n), dim3(kdbsf::TPB), 0, call.st, d_vecs, (const double *)L, nbins,
                           (const kdbsf::Target *)d_targets, kdbselect::pass_shift(pass), kdbselect::pass_width(pass), d_hist);
        HIP_TRY(hipGetLastError());
        HIP_TRY(call.end());
        HIP_TRY(hipMemcpyAsync(hist.data(), d_hist, hist_bytes, hipMemcpyDeviceToHost, call.st));
        HIP_TRY(hipStreamSynchronize(call.st));
        HIP_TRY(call.elapsed());
        for (int j = 0; j < n; j++)
            if (!sel[j].step(&hist[(size_t)j * 2 * NB], &hist[(size_t)j * 2 * NB + NB], pass))
                return fail(KDB_ERR_STATE, "kdb_size_factors: pass %d of the select found no element of the wanted rank in vector %d: the vectors changed during the call", pass, j);
    }
    for (int j = 0; j < n; j++) log_sf_out[j] = kdbselect::median_of(sel[j].low(), sel[j].high());
    if (kernel_ms_out) *kernel_ms_out = call.ms;
    return KDB_OK;
}

int kdb_scale_counts(int device_id, const void *d_vector, uint64_t nbins, double size_factor, void *d_out, int as_float64, double *kernel_ms_out)
{
    if (!d_vector || !d_out) return fail(KDB_ERR_ARG, "kdb_scale_counts: a vector is NULL");
    if ((((uintptr_t)d_vector | (uintptr_t)d_out) & 15u) != 0) return fail(KDB_ERR_ARG, "kdb_scale_counts: a vector is not 16-byte aligned");
    if (nbins == 0 || nbins > kdbsf::NBINS_MAX) return fail(KDB_ERR_ARG, "kdb_scale_counts: nbins is 0 or above 2^36 (64 x 4^17: more than a device holds)");
    if (!(size_factor > 0.0) || !std::isfinite(size_factor)) return fail(KDB_ERR_ARG, "kdb_scale_counts: the size factor %g is not finite and positive", size_factor);
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    uint32_t *d_flag = call.alloc<uint32_t>(1);
    if (!d_flag) return fail(KDB_ERR_NOMEM, "kdb_scale_counts: no room for the flag word");
    const uint32_t gx = sizefactor_grid(nbins);
    const unsigned long long *x = (const unsigned long long *)d_vector;
    uint32_t flag = 0;
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), call.st));
    HIP_TRY(call.begin());
    // x < 2^64 rounds to at most 2^64: only a size factor of 2 or less can bring a quotient to 2^63.  Then a first sweep looks and writes
    // nothing, so that a refused call leaves d_out (which may be the input) as it was.
    if (!as_float64 && size_factor <= 2.0) {
        hipLaunchKernelGGL(kdbsf::scale_kernel, dim3(gx), dim3(kdbsf::TPB), 0, call.st, x, nbins, size_factor, d_out, 0, 0, d_flag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
        HIP_TRY(hipStreamSynchronize(call.st));
        if (flag != 0) return fail(KDB_ERR_ARG, "kdb_scale_counts: a count divided by the size factor %g reaches 2^63: it has no place in an int64 matrix", size_factor);
    }
    hipLaunchKernelGGL(kdbsf::scale_kernel, dim3(gx), dim3(kdbsf::TPB), 0, call.st, x, nbins, size_factor, d_out, as_float64 ? 1 : 0, 1, d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    return KDB_OK;
}

// ---- abundance spectrum and doubled mid-ranks of a finished vector (kdb_spectrum.hip.h, kdb_spectrum_host.cpp.h) ----
int kdb_spectrum(int device_id, const void *d_vector, uint64_t nbins, uint64_t *dense_out, uint64_t *over_values_out, uint64_t over_cap,
                 uint64_t *n_over_out, double *kernel_ms_out)
{
    if (n_over_out) *n_over_out = 0;
    if (!dense_out || !n_over_out) return fail(KDB_ERR_ARG, "kdb_spectrum: dense_out and n_over_out must not be NULL");
    if (int rc = spectrum_check_args("kdb_spectrum", d_vector, nbins)) return rc;
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;
    SpectrumScratch sc;
    if (int rc = spectrum_alloc("kdb_spectrum", call, sc, over_values_out ? std::min(over_cap, nbins) : 0)) return rc;
    std::vector<uint64_t> host;
    if (int rc = spectrum_sweep(call, sc, d_vector, nbins, host)) return rc;
    const uint64_t n_over = host[kdbspectrum::DENSE];
    memcpy(dense_out, host.data(), kdbspectrum::DENSE * 8ull);
    *n_over_out = n_over;
    if (kernel_ms_out) *kernel_ms_out = call.ms;
    if (!over_values_out || n_over == 0) return KDB_OK;
    if (n_over > over_cap) return fail(KDB_ERR_ARG, "kdb_spectrum: %llu values of 65536 and above do not fit the %llu entries given", (unsigned long long)n_over, (unsigned long long)over_cap);
    HIP_TRY(hipMemcpy(over_values_out, sc.over, n_over * 8ull, hipMemcpyDeviceToHost));
    return KDB_OK;
}

int kdb_rank_transform(int device_id, const void *d_vector, uint64_t nbins, void *d_ranks_out, double *kernel_ms_out)
{
    if (nbins >= (1ull << 32)) return fail(KDB_ERR_ARG, "kdb_rank_transform: nbins is 2^32 or more (k >= 16): the doubled ranks sum to N (N + 1), which kdb_gram needs below 2^64");
    if (!d_ranks_out || ((uintptr_t)d_ranks_out & 15u) != 0) return fail(KDB_ERR_ARG, "kdb_rank_transform: the output is NULL or not 16-byte aligned");
    if (int rc = spectrum_check_args("kdb_rank_transform", d_vector, nbins)) return rc;
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;
    SpectrumScratch sc;
    std::vector<uint64_t> host;
    // the list is short on count profiles (at most Sum counts / 65536 values): a first guess, and a second sweep with the exact length where it was wrong
    if (int rc = spectrum_alloc("kdb_rank_transform", call, sc, std::min<uint64_t>(nbins, KDB_SPECTRUM_LIST_GUESS))) return rc;
    if (int rc = spectrum_sweep(call, sc, d_vector, nbins, host)) return rc;
    if (host[kdbspectrum::DENSE] > sc.cap) {
        if (int rc = spectrum_alloc("kdb_rank_transform", call, sc, host[kdbspectrum::DENSE])) return rc;
        if (int rc = spectrum_sweep(call, sc, d_vector, nbins, host)) return rc;
        if (host[kdbspectrum::DENSE] > sc.cap) return fail(KDB_ERR_STATE, "kdb_rank_transform: the vector changed during the call");
    }
    const uint64_t n_over = host[kdbspectrum::DENSE];
    std::vector<uint64_t> over(n_over);
    if (n_over) HIP_TRY(hipMemcpy(over.data(), sc.over, n_over * 8ull, hipMemcpyDeviceToHost));
    kdbspectrum_host::RankTables t;
    kdbspectrum_host::rank_tables(host.data(), kdbspectrum::DENSE, over.data(), n_over, t);
    if (t.nbins != nbins) return fail(KDB_ERR_HIP, "kdb_rank_transform: the rank tables cover %llu bins of %llu", (unsigned long long)t.nbins, (unsigned long long)nbins);
    const uint64_t nd = t.over_values.size();
    // the dense rank table, the distinct overflow values, their ranks
    unsigned long long *tables = call.alloc<unsigned long long>(kdbspectrum::DENSE + 2 * nd);
    if (!tables) return fail(KDB_ERR_NOMEM, "kdb_rank_transform: no room for the rank tables of %llu large values", (unsigned long long)nd);
    HIP_TRY(hipMemcpyAsync(tables, t.rank_dense.data(), kdbspectrum::DENSE * 8ull, hipMemcpyHostToDevice, call.st));
    if (nd) {
        HIP_TRY(hipMemcpyAsync(tables + kdbspectrum::DENSE, t.over_values.data(), nd * 8ull, hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(tables + kdbspectrum::DENSE + nd, t.over_ranks.data(), nd * 8ull, hipMemcpyHostToDevice, call.st));
    }
    const kdbspectrum::RankTables dt{tables, tables + kdbspectrum::DENSE, tables + kdbspectrum::DENSE + nd, (uint32_t)nd};
    const uint64_t nchunks = nbins / kdbspectrum::CHUNK_BINS;
    HIP_TRY(call.begin());
    hipLaunchKernelGGL(kdbspectrum::rank_map_kernel, dim3(kdbspectrum::spectrum_grid(nchunks)), dim3(kdbspectrum::TPB), 0, call.st,
                       (const unsigned long long *)d_vector, nbins, nchunks, dt, (unsigned long long *)d_ranks_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    return KDB_OK;
}

int kdb_strand_merge(int device_id, void *d_fwd, void *d_table, int k)
{
    if (k < 1 || k > 17) return fail(KDB_ERR_ARG, "kdb_strand_merge: k=%d outside 1..17", k);
    if (!d_fwd || !d_table || d_fwd == d_table) return fail(KDB_ERR_ARG, "kdb_strand_merge: d_fwd and d_table must be two vectors");
    if ((((uintptr_t)d_fwd | (uintptr_t)d_table) & 7u) != 0) return fail(KDB_ERR_ARG, "kdb_strand_merge: the vectors must be 8-byte aligned");
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;
    kdbstrands::strand_merge_launch(call.st, (unsigned long long *)d_fwd, (unsigned long long *)d_table, k);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(call.st));
    return KDB_OK;
}

// ---- reads scored against a profile (kdb_score.hip.h) ----
int kdb_score_reads(int device_id, const void *d_vector, int k, int canonical, uint64_t total, uint64_t pseudocount, const uint8_t *bases, size_t nbytes,
                    const uint64_t *offs, size_t nreads, int flags, double *log10_p_out, uint64_t *windows_out, uint64_t *zero_windows_out,
                    uint64_t *min_count_out, double *kernel_ms_out)
{
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (k < 1 || k > 17) return fail(KDB_ERR_ARG, "kdb_score_reads: k=%d out of range 1..17", k);
    if (!d_vector || ((uintptr_t)d_vector & 15u) != 0) return fail(KDB_ERR_ARG, "kdb_score_reads: the vector is NULL or not 16-byte aligned");
    if (flags & ~(KDB_SCORE_CONTINUES | KDB_SCORE_NONE_SCORED)) return fail(KDB_ERR_ARG, "kdb_score_reads: unknown flags %d", flags);
    if ((flags & KDB_SCORE_NONE_SCORED) && !(flags & KDB_SCORE_CONTINUES))
        return fail(KDB_ERR_ARG, "kdb_score_reads: KDB_SCORE_NONE_SCORED needs KDB_SCORE_CONTINUES");
    if (total == 0) return fail(KDB_ERR_ARG, "kdb_score_reads: total is 0 (an empty profile gives no probabilities)");
    const uint64_t nbins = 1ull << (2 * k);
    const unsigned __int128 total2 = (unsigned __int128)total + (unsigned __int128)pseudocount * nbins;
    if ((total2 >> 64) != 0 || pseudocount >= (1ull << 62))
        return fail(KDB_ERR_ARG, "kdb_score_reads: total + pseudocount * 4^k and 4 * pseudocount must stay below 2^64");
    if (int rc = record_check_args("kdb_score_reads", bases, nbytes, offs, nreads, log10_p_out && windows_out && zero_windows_out && min_count_out)) return rc;
    if (nreads == 0) return KDB_OK;
    if (int rc = record_check_sizes("kdb_score_reads", nbytes, nreads)) return rc;
    const bool continues = (flags & KDB_SCORE_CONTINUES) != 0;
    const bool scored_before = continues && !(flags & KDB_SCORE_NONE_SCORED);     // record 0's first scored window is a transition
    // the layout, and with it every address the kernels form, is settled here: the offsets are host memory
    kdbplan::ScoreLayout lay;
    if (const kdbplan::LayoutError bad = kdbplan::score_layout(offs, nreads, nbytes, k, kdbscore::PIECE, continues, lay)) return record_offsets_fail(bad);
    if (lay.nshort) return fail(KDB_ERR_SHORT_READ, "%llu record(s) shorter than k=%d (reference: kmer.py:461-463 raises)", (unsigned long long)lay.nshort, k);
    const uint64_t npieces = lay.npieces;
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    RecordBatch in;
    const bool staged = in.alloc(call, nbytes, nreads, lay, 32);                       // (piece_kernel's aligned words reach 23 bytes past a window's start)
    auto *pieces = call.alloc<kdbscore::PieceOut>(npieces);
    auto *ctr = call.alloc<kdb::DevCounters>(1);
    auto *log10_p = call.alloc<double>(nreads);
    auto *ints = call.alloc<unsigned long long>(3 * nreads);
    if (!staged || !pieces || !ctr || !log10_p || !ints)
        return fail(KDB_ERR_NOMEM, "kdb_score_reads: no room for the scratch of %zu residues in %zu records", nbytes, nreads);
    kdb::DevCounters c;
    memset(&c, 0, sizeof c);
    c.sus_count = 1;                       // more than sus_cap = 0: resolve_suspects_kernel judges every residue of the batch itself
    if (int rc = in.upload(call, bases, nbytes, offs, nreads, lay)) return rc;
    HIP_TRY(hipMemcpyAsync(ctr, &c, sizeof c, hipMemcpyHostToDevice, call.st));
    HIP_TRY(call.begin());
    // what kdb_window_ids refuses: bytes with bit 7 set, letters outside ACGTN that no N shields (kmer.py:309 / :170)
    hipLaunchKernelGGL(kdb::hibit_check_kernel, dim3(1024), dim3(256), 0, call.st, (const uint8_t *)in.bases, (uint64_t)nbytes, ctr);
    const unsigned check_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(2048, (nbytes / 64 + 255) / 256));
    hipLaunchKernelGGL(kdb::resolve_suspects_kernel, dim3(check_grid), dim3(256), 0, call.st, (const uint8_t *)in.bases, (uint64_t)nbytes, (const uint64_t *)in.offs,
                       (uint64_t)nreads, k, ctr, 0);
    hipLaunchKernelGGL(kdbscore::piece_kernel, dim3((unsigned)((npieces + kdbscore::TPB / 64 - 1) / (kdbscore::TPB / 64))), dim3(kdbscore::TPB), 0, call.st,
                       (const uint8_t *)in.bases, (const uint64_t *)in.offs, (const uint32_t *)in.piece_rec, (const uint32_t *)in.rec_piece0, (uint32_t)npieces,
                       (const unsigned long long *)d_vector, k, canonical ? 1 : 0, (unsigned long long)pseudocount, pieces);
    hipLaunchKernelGGL(kdbscore::record_kernel, dim3((unsigned)((nreads + 255) / 256)), dim3(256), 0, call.st, (const kdbscore::PieceOut *)pieces,
                       (const uint32_t *)in.rec_piece0, (uint64_t)nreads, (double)(uint64_t)total2, scored_before ? 1 : 0, log10_p, ints, ints + nreads, ints + 2 * nreads);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    HIP_TRY(hipMemcpyAsync(&c, ctr, sizeof c, hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    if (c.n_bad) return fail(KDB_ERR_BAD_RESIDUE, "%llu residue(s) outside ACGTN (reference: kmer.py:309 / :170 raises)", c.n_bad);
    HIP_TRY(hipMemcpy(log10_p_out, log10_p, nreads * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(windows_out, ints, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(zero_windows_out, ints + nreads, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(min_count_out, ints + 2 * nreads, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return KDB_OK;
}

// ---- one k-mer table per record (kdb_tables.hip.h) ----
int kdb_record_tables(int device_id, int k, int stride, int canonical, uint64_t phase, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads,
                      int flags, uint32_t *tables_out, uint64_t *windows_out, uint64_t *skipped_out, int32_t *first_id_out, int32_t *last_id_out,
                      double *kernel_ms_out)
{
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (k < 1 || k > kdbtables::MAX_K) return fail(KDB_ERR_ARG, "kdb_record_tables: k=%d out of range 1..%d", k, kdbtables::MAX_K);
    if (stride < 1 || stride > k) return fail(KDB_ERR_ARG, "kdb_record_tables: stride=%d out of range 1..k=%d", stride, k);
    if (flags & ~KDB_TABLES_CONTINUES) return fail(KDB_ERR_ARG, "kdb_record_tables: unknown flags %d", flags);
    const bool continues = (flags & KDB_TABLES_CONTINUES) != 0;
    if (phase >= (uint64_t)stride) return fail(KDB_ERR_ARG, "kdb_record_tables: phase=%llu must be below stride=%d", (unsigned long long)phase, stride);
    if (phase != 0 && !continues) return fail(KDB_ERR_ARG, "kdb_record_tables: a phase needs KDB_TABLES_CONTINUES");
    if (int rc = record_check_args("kdb_record_tables", bases, nbytes, offs, nreads, tables_out && windows_out && skipped_out && first_id_out && last_id_out)) return rc;
    if (nreads == 0) return KDB_OK;
    if (int rc = record_check_sizes("kdb_record_tables", nbytes, nreads)) return rc;
    // the layout, and with it every address the kernels form, is settled here: the offsets are host memory
    kdbplan::TablesLayout lay;
    if (const kdbplan::LayoutError bad = kdbplan::tables_layout(offs, nreads, nbytes, k, stride, phase, kdbtables::PIECE, 1ull << 31, lay))
        return bad != kdbplan::LAYOUT_ENTRIES ? record_offsets_fail(bad)
                                              : fail(KDB_ERR_ARG, "kdb_record_tables: more than 2^31 table entries (records x 4^k) in one call");
    // so are the residues: every byte is one of ACGTN, or nothing is launched
    if (const uint64_t nbad = residues_outside_acgtn(bases, nbytes)) return fail(KDB_ERR_BAD_RESIDUE, "kdb_record_tables: %llu residue(s) outside ACGTN", (unsigned long long)nbad);
    const uint64_t npieces = lay.npieces, nbins = 1ull << (2 * k), nmulti = lay.multi.size();
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    RecordBatch in;
    const bool staged = in.alloc(call, nbytes, nreads, lay, 32);                       // (tables_piece_kernel's aligned words reach 15 bytes past a window's start)
    auto *multi = nmulti ? call.alloc<uint32_t>(nmulti) : nullptr;
    auto *pieces = call.alloc<kdbtables::PieceOut>(npieces);
    auto *tables = call.alloc<uint32_t>(nreads * nbins);
    auto *counts = call.alloc<unsigned long long>(2 * nreads);
    auto *ends = call.alloc<int32_t>(2 * nreads);
    if (!staged || (nmulti && !multi) || !pieces || !tables || !counts || !ends)
        return fail(KDB_ERR_NOMEM, "kdb_record_tables: no room for the scratch of %zu residues in %zu records of 4^%d entries", nbytes, nreads, k);
    if (int rc = in.upload(call, bases, nbytes, offs, nreads, lay)) return rc;
    if (nmulti) HIP_TRY(hipMemcpyAsync(multi, lay.multi.data(), nmulti * sizeof(uint32_t), hipMemcpyHostToDevice, call.st));
    HIP_TRY(call.begin());
    if (nmulti)
        hipLaunchKernelGGL(kdbtables::tables_zero_kernel, dim3((unsigned)std::min<uint64_t>(nmulti, 4096)), dim3(256), 0, call.st, (const uint32_t *)multi,
                           (uint32_t)nmulti, k, tables);
    hipLaunchKernelGGL(kdbtables::tables_piece_kernel, dim3((unsigned)((npieces + kdbtables::WAVES - 1) / kdbtables::WAVES)), dim3(kdbtables::TPB),
                       kdbtables::lds_bytes(k), call.st, (const uint8_t *)in.bases, (const uint64_t *)in.offs, (const uint32_t *)in.piece_rec,
                       (const uint32_t *)in.rec_piece0, (uint32_t)npieces, k, stride, canonical ? 1 : 0, (uint32_t)phase, tables, pieces);
    hipLaunchKernelGGL(kdbtables::tables_record_kernel, dim3((unsigned)((nreads + 255) / 256)), dim3(256), 0, call.st, (const kdbtables::PieceOut *)pieces,
                       (const uint32_t *)in.rec_piece0, (uint64_t)nreads, counts, counts + nreads, ends, ends + nreads);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    HIP_TRY(hipMemcpyAsync(tables_out, tables, nreads * nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipMemcpyAsync(windows_out, counts, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipMemcpyAsync(skipped_out, counts + nreads, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipMemcpyAsync(first_id_out, ends, nreads * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipMemcpyAsync(last_id_out, ends + nreads, nreads * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    return KDB_OK;
}

// ---- the (w,k)-minimizers of every record (kdb_minimizers.hip.h) ----
int kdb_minimizers(int device_id, int k, int w, int canonical, int order, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads,
                   uint64_t *counts_out, uint64_t *ids_out, uint32_t *pos_out, uint8_t *strand_out, size_t cap, uint64_t *total_out, double *kernel_ms_out)
{
    namespace km = kdbminimizers;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (k < 1 || k > km::MAX_K) return fail(KDB_ERR_ARG, "kdb_minimizers: k=%d out of range 1..%d", k, km::MAX_K);
    if (w < 1 || w > km::MAX_W) return fail(KDB_ERR_ARG, "kdb_minimizers: w=%d out of range 1..%d", w, km::MAX_W);
    if (order != KDB_MINIMIZER_LEX && order != KDB_MINIMIZER_HASHED) return fail(KDB_ERR_ARG, "kdb_minimizers: unknown order %d", order);
    if (!total_out) return fail(KDB_ERR_ARG, "kdb_minimizers: total_out must not be NULL");
    if (int rc = record_check_args("kdb_minimizers", bases, nbytes, offs, nreads, counts_out != nullptr)) return rc;
    if (nreads == 0) {
        *total_out = 0;
        return KDB_OK;
    }
    if (cap > 0 && (!ids_out || !pos_out)) return fail(KDB_ERR_ARG, "kdb_minimizers: ids_out and pos_out must not be NULL where cap > 0");
    if (int rc = record_check_sizes("kdb_minimizers", nbytes, nreads)) return rc;
    // the layout, and with it every address the kernels form, is settled here: the offsets are host memory
    kdbplan::MinimizersLayout lay;
    if (const kdbplan::LayoutError bad = kdbplan::minimizers_layout(offs, nreads, nbytes, k, (uint32_t)w, km::PIECE, lay)) return record_offsets_fail(bad);
    // so are the residues: every byte is one of ACGTN, or nothing is launched
    if (const uint64_t nbad = residues_outside_acgtn(bases, nbytes)) return fail(KDB_ERR_BAD_RESIDUE, "kdb_minimizers: %llu residue(s) outside ACGTN", (unsigned long long)nbad);
    const uint32_t npieces = (uint32_t)lay.npieces, nblocks = (npieces + km::SCAN_BLOCK - 1) / km::SCAN_BLOCK;
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    // (select_kernel's aligned words reach 3 bytes past a record's end, emit_kernel's five 39 bytes past a window's start)
    RecordBatch in;
    const bool staged = in.alloc(call, nbytes, nreads, lay, 64);
    auto *flags = call.alloc<uint8_t>(nbytes + 16);
    auto *piece_count = call.alloc<uint32_t>(npieces), *piece_off = call.alloc<uint32_t>((uint64_t)npieces + 1), *sums = call.alloc<uint32_t>(nblocks);
    auto *counts = call.alloc<unsigned long long>(nreads);
    if (!staged || !flags || !piece_count || !piece_off || !sums || !counts)
        return fail(KDB_ERR_NOMEM, "kdb_minimizers: no room for the scratch of %zu residues in %zu records", nbytes, nreads);
    if (int rc = in.upload(call, bases, nbytes, offs, nreads, lay)) return rc;
    const dim3 piece_grid((npieces + km::WAVES - 1) / km::WAVES);
    uint32_t total = 0;
    HIP_TRY(call.begin());
    hipLaunchKernelGGL(km::select_kernel, piece_grid, dim3(km::TPB), (size_t)km::WAVES * lay.lds_wave, call.st, (const uint8_t *)in.bases, (const uint64_t *)in.offs,
                       (const uint32_t *)in.piece_rec, (const uint32_t *)in.rec_piece0, npieces, k, (uint32_t)w, canonical ? 1 : 0, order, lay.max_keys, lay.lds_wave, flags,
                       piece_count);
    hipLaunchKernelGGL(km::scan_sums_kernel, dim3(nblocks), dim3(km::SCAN_TPB), 0, call.st, (const uint32_t *)piece_count, npieces, sums);
    hipLaunchKernelGGL(km::scan_top_kernel, dim3(1), dim3(km::SCAN_TPB), 0, call.st, sums, nblocks, piece_off + npieces);
    hipLaunchKernelGGL(km::scan_apply_kernel, dim3(nblocks), dim3(km::SCAN_TPB), 0, call.st, (const uint32_t *)piece_count, npieces, (const uint32_t *)sums, piece_off);
    hipLaunchKernelGGL(km::record_counts_kernel, dim3((unsigned)((nreads + 255) / 256)), dim3(256), 0, call.st, (const uint32_t *)piece_off,
                       (const uint32_t *)in.rec_piece0, (uint64_t)nreads, counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    HIP_TRY(hipMemcpyAsync(&total, piece_off + npieces, sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    // the lists, where the caller's arrays hold them
    uint64_t *d_ids = nullptr;
    uint32_t *d_pos = nullptr;
    uint8_t *d_strand = nullptr;
    const bool emit = total > 0 && (uint64_t)total <= (uint64_t)cap;
    if (emit) {
        d_ids = call.alloc<uint64_t>(total);
        d_pos = call.alloc<uint32_t>(total);
        d_strand = strand_out ? call.alloc<uint8_t>(total) : nullptr;
        if (!d_ids || !d_pos || (strand_out && !d_strand)) return fail(KDB_ERR_NOMEM, "kdb_minimizers: no room for the lists of %u minimizers", total);
        HIP_TRY(call.begin());
        hipLaunchKernelGGL(km::emit_kernel, piece_grid, dim3(km::TPB), 0, call.st, (const uint8_t *)in.bases, (const uint64_t *)in.offs, (const uint32_t *)in.piece_rec,
                           (const uint32_t *)in.rec_piece0, npieces, k, canonical ? 1 : 0, (const uint8_t *)flags, (const uint32_t *)piece_off, (unsigned long long *)d_ids,
                           d_pos, d_strand);
        HIP_TRY(hipGetLastError());
        HIP_TRY(call.end());
        HIP_TRY(hipMemcpyAsync(ids_out, d_ids, (size_t)total * sizeof(uint64_t), hipMemcpyDeviceToHost, call.st));
        HIP_TRY(hipMemcpyAsync(pos_out, d_pos, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
        if (strand_out) HIP_TRY(hipMemcpyAsync(strand_out, d_strand, (size_t)total, hipMemcpyDeviceToHost, call.st));
    }
    HIP_TRY(hipMemcpyAsync(counts_out, counts, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    if (emit) HIP_TRY(call.elapsed(kernel_ms_out));
    *total_out = total;
    return KDB_OK;
}

// ---- banded local alignments, a wave per task (kdb_align.hip.h), and their traceback (kdb_align_trace.hip.h) ----
}  // extern "C"

namespace {

// what kdb_align_banded and kdb_align_traceback take alike
struct AlignArgs {
    const uint8_t *q_bases;
    size_t q_nbytes;
    const uint64_t *q_offs;
    size_t nq;
    const uint8_t *r_bases;
    size_t r_nbytes;
    const uint64_t *r_offs;
    size_t nr;
    const uint32_t *task_q, *task_r;
    const int64_t *task_diag;
    const uint8_t *task_strand;
    size_t ntasks;
    int band, match, mismatch, gap_open, gap_extend;
    int32_t *score_out;
    uint32_t *qstart_out, *qend_out, *rstart_out, *rend_out;
};

int align_check_scalars(const char *who, const AlignArgs &a)
{
    if (a.band < 1 || a.band > kdbalign::MAX_BAND) return fail(KDB_ERR_ARG, "%s: band=%d out of range 1..%d", who, a.band, kdbalign::MAX_BAND);
    if (a.match < 1 || a.match > 127) return fail(KDB_ERR_ARG, "%s: match=%d out of range 1..127", who, a.match);
    if (a.mismatch < -127 || a.mismatch > 0 || a.gap_open < -127 || a.gap_open > 0 || a.gap_extend < -127 || a.gap_extend > 0)
        return fail(KDB_ERR_ARG, "%s: mismatch=%d, gap_open=%d, gap_extend=%d: each must lie in -127..0", who, a.mismatch, a.gap_open, a.gap_extend);
    return KDB_OK;
}

// everything about a batch of ntasks >= 1 tasks that is settled on the host: every address the kernels form (the offsets and the tasks
// are host memory) and every residue
int align_check_batch(const char *who, const AlignArgs &a, kdbplan::AlignLayout &lay)
{
    namespace ka = kdbalign;
    if (!a.q_offs || !a.r_offs || (!a.q_bases && a.q_nbytes) || (!a.r_bases && a.r_nbytes) || !a.task_q || !a.task_r || !a.task_diag || !a.task_strand || !a.score_out ||
        !a.qstart_out || !a.qend_out || !a.rstart_out || !a.rend_out)
        return fail(KDB_ERR_ARG, "%s: NULL buffer", who);
    if (a.q_nbytes > (1ull << 30) || a.r_nbytes > (1ull << 30)) return fail(KDB_ERR_ARG, "%s: at most 2^30 residues per buffer", who);
    if (a.nq > (1ull << 30) || a.nr > (1ull << 30)) return fail(KDB_ERR_ARG, "%s: at most 2^30 records per buffer", who);
    if (a.ntasks > (1ull << 26)) return fail(KDB_ERR_ARG, "%s: at most 2^26 tasks per call", who);
    if (const kdbplan::LayoutError bad = kdbplan::align_layout(a.q_offs, a.nq, a.q_nbytes, a.r_offs, a.nr, a.r_nbytes, a.task_q, a.task_r, a.task_diag, a.task_strand,
                                                               a.ntasks, (uint32_t)a.band, ka::MAX_QUERY, ka::WAVES, ka::GRID_MAX, lay)) {
        if (bad == kdbplan::LAYOUT_ENDS) return fail(KDB_ERR_ARG, "%s: offsets must start at 0 and end at the buffer's size", who);
        if (bad == kdbplan::LAYOUT_RISE) return fail(KDB_ERR_ARG, "%s: offsets must rise from 0 to the buffer's size", who);
        if (bad == kdbplan::LAYOUT_TASK) return fail(KDB_ERR_ARG, "%s: task %llu names a record that is not there", who, (unsigned long long)lay.bad);
        if (bad == kdbplan::LAYOUT_STRAND) return fail(KDB_ERR_ARG, "%s: task %llu has a strand that is neither 0 nor 1", who, (unsigned long long)lay.bad);
        return fail(KDB_ERR_ARG, "%s: the query of task %llu holds more than 2^20 residues", who, (unsigned long long)lay.bad);
    }
    // so are the residues: every byte is one of ACGTN, or nothing is launched
    if (const uint64_t nbad = residues_outside_acgtn(a.q_bases, a.q_nbytes) + residues_outside_acgtn(a.r_bases, a.r_nbytes))
        return fail(KDB_ERR_BAD_RESIDUE, "%s: %llu residue(s) outside ACGTN", who, (unsigned long long)nbad);
    return KDB_OK;
}

// the batch on the device: the residues as whole words, the offsets, the tasks and the five outputs per task
struct AlignBatch {
    uint64_t q_nwords = 0, r_nwords = 0;
    uint32_t *q = nullptr, *r = nullptr, *tq = nullptr, *tr = nullptr, *out = nullptr;
    uint64_t *qoffs = nullptr, *roffs = nullptr;
    int64_t *diag = nullptr;
    uint8_t *strand = nullptr;

    bool alloc(AnalysisCall &call, const AlignArgs &a)
    {
        q_nwords = (a.q_nbytes + 3) / 4, r_nwords = (a.r_nbytes + 3) / 4;                            // (the kernels read whole words, and none outside these)
        q = call.alloc<uint32_t>(q_nwords + 4), r = call.alloc<uint32_t>(r_nwords + 4);
        qoffs = call.alloc<uint64_t>(a.nq + 1), roffs = call.alloc<uint64_t>(a.nr + 1);
        tq = call.alloc<uint32_t>(a.ntasks), tr = call.alloc<uint32_t>(a.ntasks);
        diag = call.alloc<int64_t>(a.ntasks);
        strand = call.alloc<uint8_t>(a.ntasks);
        out = call.alloc<uint32_t>(5 * (uint64_t)a.ntasks);
        return q && r && qoffs && roffs && tq && tr && diag && strand && out;
    }
    int upload(AnalysisCall &call, const AlignArgs &a)
    {
        if (a.q_nbytes) HIP_TRY(hipMemcpyAsync(q, a.q_bases, a.q_nbytes, hipMemcpyHostToDevice, call.st));
        if (a.r_nbytes) HIP_TRY(hipMemcpyAsync(r, a.r_bases, a.r_nbytes, hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(qoffs, a.q_offs, (a.nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(roffs, a.r_offs, (a.nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(tq, a.task_q, a.ntasks * sizeof(uint32_t), hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(tr, a.task_r, a.ntasks * sizeof(uint32_t), hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(diag, a.task_diag, a.ntasks * sizeof(int64_t), hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(strand, a.task_strand, a.ntasks, hipMemcpyHostToDevice, call.st));
        return KDB_OK;
    }
    uint32_t *column(const AlignArgs &a, int x) const { return out + (uint64_t)x * a.ntasks; }       // score, qstart, qend, rstart, rend
    int download(AnalysisCall &call, const AlignArgs &a)
    {
        HIP_TRY(hipMemcpyAsync(a.score_out, column(a, 0), a.ntasks * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
        HIP_TRY(hipMemcpyAsync(a.qstart_out, column(a, 1), a.ntasks * sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
        HIP_TRY(hipMemcpyAsync(a.qend_out, column(a, 2), a.ntasks * sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
        HIP_TRY(hipMemcpyAsync(a.rstart_out, column(a, 3), a.ntasks * sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
        HIP_TRY(hipMemcpyAsync(a.rend_out, column(a, 4), a.ntasks * sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
        return KDB_OK;
    }
};

}  // namespace

extern "C" {

int kdb_align_banded(int device_id, const uint8_t *q_bases, size_t q_nbytes, const uint64_t *q_offs, size_t nq, const uint8_t *r_bases, size_t r_nbytes,
                     const uint64_t *r_offs, size_t nr, const uint32_t *task_q, const uint32_t *task_r, const int64_t *task_diag, const uint8_t *task_strand,
                     size_t ntasks, int band, int match, int mismatch, int gap_open, int gap_extend, int32_t *score_out, uint32_t *qstart_out, uint32_t *qend_out,
                     uint32_t *rstart_out, uint32_t *rend_out, double *kernel_ms_out)
{
    namespace ka = kdbalign;
    const char *const who = "kdb_align_banded";
    const AlignArgs a{q_bases, q_nbytes, q_offs, nq, r_bases, r_nbytes, r_offs, nr, task_q, task_r, task_diag, task_strand, ntasks, band, match, mismatch, gap_open,
                      gap_extend, score_out, qstart_out, qend_out, rstart_out, rend_out};
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (int rc = align_check_scalars(who, a)) return rc;
    if (ntasks == 0) return KDB_OK;
    kdbplan::AlignLayout lay;
    if (int rc = align_check_batch(who, a, lay)) return rc;
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    AlignBatch in;
    if (!in.alloc(call, a)) return fail(KDB_ERR_NOMEM, "%s: no room for %zu + %zu residues and %zu tasks", who, q_nbytes, r_nbytes, ntasks);
    if (int rc = in.upload(call, a)) return rc;
    HIP_TRY(call.begin());
    hipLaunchKernelGGL(ka::align_kernel, dim3(lay.grid), dim3(ka::TPB), (size_t)ka::WAVES * kdbplan::align_lds_wave(ka::STAGE), call.st, (const uint32_t *)in.q,
                       (int64_t)in.q_nwords, (const uint64_t *)in.qoffs, (const uint32_t *)in.r, (int64_t)in.r_nwords, (const uint64_t *)in.roffs, (const uint32_t *)in.tq,
                       (const uint32_t *)in.tr, (const int64_t *)in.diag, (const uint8_t *)in.strand, (uint32_t)ntasks, band, match, mismatch, gap_open, gap_extend,
                       (int32_t *)in.column(a, 0), in.column(a, 1), in.column(a, 2), in.column(a, 3), in.column(a, 4));
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.end());
    if (int rc = in.download(call, a)) return rc;
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    return KDB_OK;
}

int kdb_align_traceback(int device_id, const uint8_t *q_bases, size_t q_nbytes, const uint64_t *q_offs, size_t nq, const uint8_t *r_bases, size_t r_nbytes,
                        const uint64_t *r_offs, size_t nr, const uint32_t *task_q, const uint32_t *task_r, const int64_t *task_diag, const uint8_t *task_strand,
                        size_t ntasks, int band, int match, int mismatch, int gap_open, int gap_extend, size_t scratch_limit, int32_t *score_out, uint32_t *qstart_out,
                        uint32_t *qend_out, uint32_t *rstart_out, uint32_t *rend_out, uint64_t *nruns_out, uint32_t *runs_out, size_t cap, uint64_t *total_out,
                        double *kernel_ms_out)
{
    namespace ka = kdbalign;
    const char *const who = "kdb_align_traceback";
    const AlignArgs a{q_bases, q_nbytes, q_offs, nq, r_bases, r_nbytes, r_offs, nr, task_q, task_r, task_diag, task_strand, ntasks, band, match, mismatch, gap_open,
                      gap_extend, score_out, qstart_out, qend_out, rstart_out, rend_out};
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (int rc = align_check_scalars(who, a)) return rc;
    if (!total_out) return fail(KDB_ERR_ARG, "%s: total_out must not be NULL", who);
    if (cap > 0 && !runs_out) return fail(KDB_ERR_ARG, "%s: runs_out must not be NULL where cap > 0", who);
    if (ntasks == 0) {
        *total_out = 0;
        return KDB_OK;
    }
    if (!nruns_out) return fail(KDB_ERR_ARG, "%s: NULL buffer", who);
    kdbplan::AlignLayout lay;
    if (int rc = align_check_batch(who, a, lay)) return rc;
    // the direction scratch of every task and the chunks the call works through, on the host as well
    std::vector<uint64_t> task_bytes(ntasks);
    for (size_t t = 0; t < ntasks; t++) {
        const uint64_t m = q_offs[task_q[t] + 1] - q_offs[task_q[t]], n = r_offs[task_r[t] + 1] - r_offs[task_r[t]];
        task_bytes[t] = kdbplan::align_trace_bytes(kdbplan::align_window(m, n, task_diag[t], (uint32_t)band), (uint32_t)band);
    }
    kdbplan::AlignTraceChunks chunks;
    kdbplan::align_trace_chunks(task_bytes.data(), ntasks, scratch_limit ? (uint64_t)scratch_limit : (uint64_t)KDB_ALIGN_TRACE_SCRATCH, chunks);
    AnalysisCall call;
    if (int rc = call.open(device_id)) return rc;

    AlignBatch in;
    const bool staged = in.alloc(call, a);
    const uint32_t scan_blocks = (uint32_t)((ntasks + ka::SCAN_BLOCK - 1) / ka::SCAN_BLOCK);
    auto *dirs = call.alloc<uint32_t>(chunks.largest / 4 + 1);
    auto *dir_offs = call.alloc<uint64_t>(ntasks), *run_offs = call.alloc<uint64_t>(ntasks), *counts64 = call.alloc<uint64_t>(ntasks);
    auto *sums = call.alloc<uint64_t>((uint64_t)scan_blocks + 1);             // (the last entry is the carry from chunk to chunk, at the end the total)
    auto *counts = call.alloc<uint32_t>(ntasks);
    auto *runs = cap ? call.alloc<uint32_t>(cap) : nullptr;
    if (!staged || !dirs || !dir_offs || !run_offs || !counts64 || !sums || !counts || (cap && !runs))
        return fail(KDB_ERR_NOMEM, "%s: no room for %zu + %zu residues, %zu tasks, %llu bytes of directions and %zu runs", who, q_nbytes, r_nbytes, ntasks,
                    (unsigned long long)chunks.largest, cap);
    if (int rc = in.upload(call, a)) return rc;
    HIP_TRY(hipMemcpyAsync(dir_offs, chunks.offs.data(), ntasks * sizeof(uint64_t), hipMemcpyHostToDevice, call.st));
    uint64_t *const carry = sums + scan_blocks;
    HIP_TRY(hipMemsetAsync(carry, 0, sizeof(uint64_t), call.st));
    const size_t lds = (size_t)ka::WAVES * kdbplan::align_lds_wave(ka::STAGE);
    HIP_TRY(call.begin());
    for (size_t k = 0; k + 1 < chunks.first.size(); k++) {
        const uint32_t lo = (uint32_t)chunks.first[k], hi = (uint32_t)chunks.first[k + 1], nchunk = hi - lo;
        const dim3 grid((unsigned)std::min<uint64_t>((nchunk + ka::WAVES - 1) / ka::WAVES, ka::GRID_MAX)), block(ka::TPB);
        const uint32_t nblocks = (nchunk + ka::SCAN_BLOCK - 1) / ka::SCAN_BLOCK;
#define KDB_TRACE_TASKS (const uint32_t *)in.q, (int64_t)in.q_nwords, (const uint64_t *)in.qoffs, (const uint32_t *)in.r, (int64_t)in.r_nwords, (const uint64_t *)in.roffs, \
                        (const uint32_t *)in.tq, (const uint32_t *)in.tr, (const int64_t *)in.diag, (const uint8_t *)in.strand, lo, hi, band
        hipLaunchKernelGGL(ka::trace_forward_kernel, grid, block, lds, call.st, KDB_TRACE_TASKS, match, mismatch, gap_open, gap_extend, (int32_t *)in.column(a, 0),
                           in.column(a, 1), in.column(a, 2), in.column(a, 3), in.column(a, 4), dirs, (const uint64_t *)dir_offs);
        hipLaunchKernelGGL(ka::walk_kernel<false>, grid, block, 0, call.st, KDB_TRACE_TASKS, (const int32_t *)in.column(a, 0), (const uint32_t *)in.column(a, 2),
                           (const uint32_t *)in.column(a, 4), (const uint32_t *)dirs, (const uint64_t *)dir_offs, counts, (const ka::u64 *)nullptr, (uint32_t *)nullptr,
                           (ka::u64)0);
        hipLaunchKernelGGL(ka::scan_sums_kernel, dim3(nblocks), dim3(ka::SCAN_TPB), 0, call.st, (const uint32_t *)counts + lo, nchunk, (ka::u64 *)sums);
        hipLaunchKernelGGL(ka::scan_top_kernel, dim3(1), dim3(ka::SCAN_TPB), 0, call.st, (ka::u64 *)sums, nblocks, (ka::u64 *)carry);
        hipLaunchKernelGGL(ka::scan_apply_kernel, dim3(nblocks), dim3(ka::SCAN_TPB), 0, call.st, (const uint32_t *)counts + lo, nchunk, (const ka::u64 *)sums,
                           (ka::u64 *)run_offs + lo, (ka::u64 *)counts64 + lo);
        // (a task whose runs do not lie inside the cap writes none: the total then exceeds the cap, and the array is not handed out)
        if (cap)
            hipLaunchKernelGGL(ka::walk_kernel<true>, grid, block, 0, call.st, KDB_TRACE_TASKS, (const int32_t *)in.column(a, 0), (const uint32_t *)in.column(a, 2),
                               (const uint32_t *)in.column(a, 4), (const uint32_t *)dirs, (const uint64_t *)dir_offs, counts, (const ka::u64 *)run_offs, runs, (ka::u64)cap);
#undef KDB_TRACE_TASKS
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(call.end());
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, carry, sizeof(uint64_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    HIP_TRY(call.elapsed(kernel_ms_out));
    if (int rc = in.download(call, a)) return rc;
    HIP_TRY(hipMemcpyAsync(nruns_out, counts64, ntasks * sizeof(uint64_t), hipMemcpyDeviceToHost, call.st));
    if (total > 0 && total <= (uint64_t)cap) HIP_TRY(hipMemcpyAsync(runs_out, runs, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    *total_out = total;
    return KDB_OK;
}

}  // extern "C"
