// kdb_engine.hip -- host side of libkdbhip.so: the C ABI of include/kdbhip.h, the
// engine object (HBM count vector, streams, pinned double-buffered staging) and
// the kernel launches.  gfx950 only; no CPU fallback: every entry point that
// needs the device fails with KDB_ERR_HIP if HIP cannot provide one.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kdbhip.h"
#include "kdb_kernels.hip.h"
#include "kdb_hist.hip.h"
#include "kdb_scatter.hip.h"
#include "kdb_scatter_host.hip.h"
#include "kdb_smallk.hip.h"
#include "kdb_probe.hip.h"
#include "kdb_gram.hip.h"
#include "kdb_pairstats.hip.h"
#include "kdb_sizefactors.hip.h"
#include "kdb_spectrum.hip.h"
#include "kdb_spectrum_host.cpp.h"
#include "kdb_strands.hip.h"
#include "kdb_score.hip.h"
#include "kdb_hostparse.cpp.h"
#include "kdb_kdbwriter.cpp.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(KDB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                        __FILE__, __LINE__);                                                  \
    } while (0)

constexpr int NBUF = 2;                                  // double-buffered staging
const char *const KERNEL_NAMES[KDB_N_KERNELS] = {
    "lens+mark_reads_kernel", "count_kernel", "scatter_bases_kernel", "scatter_ids_kernel", "pages_sort_kernels", "page_hist_kernel", "stats_kernel", "strand_merge_kernel"};

struct ProfSpan { hipEvent_t a, b; int kernel; };

// pageable -> pinned staging copy, split over a few host threads (one memcpy stream is ~10 GB/s, PCIe Gen5 is ~5x that)
void parallel_copy(uint8_t *dst, const uint8_t *src, size_t n, int nthreads)
{
    const size_t min_piece = 4u << 20;
    int t = (int)std::min<size_t>((size_t)std::max(nthreads, 1), std::max<size_t>(n / min_piece, 1));
    if (t <= 1) { if (n) memcpy(dst, src, n); return; }
    std::vector<std::thread> th;
    th.reserve((size_t)t - 1);
    const size_t piece = (n / (size_t)t + 63) & ~(size_t)63;
    for (int i = 1; i < t; i++) {
        const size_t a = std::min(n, piece * (size_t)i), b = std::min(n, piece * (size_t)(i + 1));
        if (b > a) th.emplace_back([=] { memcpy(dst + a, src + a, b - a); });
    }
    memcpy(dst, src, std::min(n, piece));
    for (auto &x : th) x.join();
}

// First touch of a fresh host buffer that is about to be overwritten whole (a np.empty() the vector is copied back into): the page
// faults of one copying thread cost 0.35 s of the 0.5 s an 8 GiB copy-back took; spread over a few threads they take a tenth.
// Writes one zero per 4 KiB page: only for buffers whose every byte is written afterwards.
void touch_pages(void *buf, size_t n, int nthreads)
{
    if (n < (64u << 20)) return;
    uint8_t *p = (uint8_t *)buf;
    const int t = std::max(1, std::min(nthreads, 64));
    std::vector<std::thread> th;
    const size_t piece = ((n / (size_t)t) + 4095) & ~(size_t)4095;
    for (int i = 0; i < t; i++) {
        const size_t a = std::min(n, piece * (size_t)i), b = std::min(n, piece * (size_t)(i + 1));
        if (b > a) th.emplace_back([=] { for (size_t o = a; o < b; o += 4096) ((volatile uint8_t *)p)[o] = 0; });
    }
    for (auto &x : th) x.join();
}

}  // namespace

struct kdb_engine {
    int k = 0, canonical = 1, n_mode = KDB_N_DROP, device = 0;
    uint64_t nbins = 0;
    unsigned long long *d_table = nullptr;
    bool owns_table = false;
    bool table_escaped = false;      // kdb_table handed the vector's address out: the caller may write it at any time
    kdb::DevCounters *d_ctr = nullptr;
    unsigned long long *d_worklist = nullptr;        // EXPAND mode: windows with > 2 N's, expanded by a workgroup each
    size_t worklist_cap = 1u << 20;
    uint32_t *d_first_rec = nullptr; size_t first_rec_cap = 0;       // record that holds every 4096th byte of the batch in hand (lens_kernel)
    unsigned long long *d_suspects = nullptr;        // DROP mode: positions of a batch's residues that are neither ACGT nor N (resolve_suspects_kernel)
    unsigned long long *sh_suspects = nullptr;       // the same for kdb_shred / kdb_window_ids
    size_t suspects_cap = 1u << 16;
    hipStream_t s_compute = nullptr, s_copy = nullptr;

    // pinned staging (allocated on first kdb_submit)
    size_t stage_bytes = 64ull << 20, stage_reads = 2ull << 20;
    uint8_t *h_bases[NBUF] = {nullptr, nullptr};
    uint64_t *h_offs[NBUF] = {nullptr, nullptr};
    uint8_t *d_bases[NBUF] = {nullptr, nullptr};
    uint64_t *d_offs[NBUF] = {nullptr, nullptr};
    hipEvent_t ev_copied[NBUF] = {nullptr, nullptr}, ev_done[NBUF] = {nullptr, nullptr};
    bool inflight[NBUF] = {false, false};
    hipEvent_t busy[NBUF] = {nullptr, nullptr};     // what must complete before staging buffer b is reused
    int next_buf = 0;
    bool staging_ready = false;
    int copy_threads = 8;

    // device-side accumulation of staged chunks (large k: every batch pays one sweep of the 4^k vector in P2,
    // so 64 MiB batches would be dominated by it; chunks are appended here and counted as one batch)
    int64_t accum_bytes = -1;                        // -1 auto (1 GiB for k >= 13, off below), 0 off
    size_t acc_cap = 0, acc_reads_cap = 0;
    uint8_t *d_acc_bases[2] = {nullptr, nullptr};
    uint64_t *d_acc_offs[2] = {nullptr, nullptr};
    hipEvent_t ev_acc_done[2] = {nullptr, nullptr};
    hipEvent_t ev_acc_copied = nullptr;
    // kdb_submit_pinned: the DMA reads the caller's buffer; call N waits for the copies of call N-2, so a caller that
    // cycles through three buffers (kmerdb_amd.reader) can never overwrite one that is still being read
    hipEvent_t ev_pin[2] = {nullptr, nullptr};
    bool pin_used[2] = {false, false};
    int pin_idx = 0;
    bool acc_inflight[2] = {false, false};
    int acc_slot = 0;
    size_t acc_nb = 0, acc_nr = 0;
    bool acc_ready = false;

    // options
    int64_t algo = 0;                 // 0 auto, 1 direct atomics, 2 LDS-histogram paths
    int min_len = 0;                  // records shorter than this are an error (0 = k)
    int smallk_old = 0;               // 1: k <= 7 through count_lds_kernel and k = 8 through the paged scatter, as before round 4 (for comparison)
    kdb::PagedOptions opt;            // tuning options of the paged-scatter paths: written by kdb_set_option alone, read by the host code of those paths
    kdb::ScatterState sc;             // scratch of the paged-scatter path (8 <= k <= 12)
    // the one-level path with the scatter kernel of batch i + 1 beside the histogram pass of batch i ("overlap" option; DROP mode)
    int overlap = 0;                  // 0 off, 1 on
    int overlap_hist_cus = 0;         // > 0: the pass's stream is masked to that many CUs and the compute stream to the others; 0: no masks
    int overlap_mask_mode = 0;        // which CUs the pass gets: 0 the first ones, 1 every (n / H)-th, 2 the first H / 8 of every 32
    bool compute_masked = false;
    hipStream_t s_hist = nullptr;
    kdb::OverlapState ov;
    kdb::TwoLevelPaged tp;            // its two-level form (k = 13..17): level-1 scratch and the arena of pending level-2 pages
    kdb::OneLevelPending ol;          // the one-level path with option one_level_defer: the arena of batches scattered but not yet added to the vector
    int64_t oom_fallbacks = 0;        // batches that fell back to direct atomics because scratch did not fit
    // canonical engines, one-level LDS-histogram paths: batches count forward ids into d_fwd, kdb_sync adds both strands to d_table
    // at the canonical bins (kdb_strands.hip.h).  d_table itself is only ever added to, at canonical bins, as without the staging.
    int strand_merge = 1;             // 0: min(fwd, rc) per window in the counting kernels, straight into d_table
    int strand_merge_max_k = 12;      // the largest k that is staged (never more than one_level_max_k); k = 13 measured no faster, DESIGN.md section 4
    unsigned long long *d_fwd = nullptr;             // 4^k uint64, allocated at the first staged batch; all zero unless strands_pending
    bool strands_pending = false;

    // ids-only engines (kdb_create_ids) have no count vector; scratch of kdb_shred / kdb_window_ids (grow-only)
    bool tableless = false;
    uint8_t *sh_seq = nullptr; size_t sh_seq_cap = 0;
    uint64_t *sh_offs = nullptr; size_t sh_offs_cap = 0;
    unsigned long long *sh_ids = nullptr; size_t sh_ids_cap = 0;
    kdb::DevCounters *sh_ctr = nullptr;

    // samplesheet accumulator (kdb_fold_file): counts = counts + counts_ stays on the device
    unsigned long long *d_acc_table = nullptr;
    uint64_t folded_files = 0, folded_total = 0;
    uint64_t d2h_bytes = 0;           // bytes of count vector copied to the host so far (tests assert "one copy at the end")
    uint64_t bytes_in = 0;            // residue bytes handed to the counting kernels so far

    // profiling
    bool prof = false;
    std::vector<ProfSpan> spans;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[KDB_N_KERNELS] = {0};
    uint64_t prof_n[KDB_N_KERNELS] = {0};
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

hipEvent_t prof_event(kdb_engine *e)
{
    hipEvent_t ev = nullptr;
    if (!e->ev_pool.empty()) { ev = e->ev_pool.back(); e->ev_pool.pop_back(); return ev; }
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return ev;
}

struct ProfScope {
    kdb_engine *e; int kernel; hipStream_t stream; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(kdb_engine *e_, int kernel_, hipStream_t stream_ = nullptr) : e(e_), kernel(kernel_), stream(stream_ ? stream_ : e_->s_compute)
    {
        if (!e->prof) return;
        a = prof_event(e); b = prof_event(e);
        if (a) (void)hipEventRecord(a, stream);
    }
    ~ProfScope()
    {
        if (!e->prof || !a || !b) return;
        (void)hipEventRecord(b, stream);
        e->spans.push_back({a, b, kernel});
    }
};

struct EngineProf : kdb::ProfHook {
    kdb_engine *e; ProfScope *cur = nullptr;
    explicit EngineProf(kdb_engine *e_) : e(e_) {}
    void begin(int kernel) override { cur = new ProfScope(e, kernel); }
    void begin_on(int kernel, hipStream_t st) override { cur = new ProfScope(e, kernel, st); }
    void end() override { delete cur; cur = nullptr; }
    ~EngineProf() override { delete cur; }
};

int prof_collect(kdb_engine *e)
{
    for (auto &s : e->spans) {
        HIP_TRY(hipEventSynchronize(s.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
        e->prof_ms[s.kernel] += ms;
        e->prof_n[s.kernel] += 1;
        e->ev_pool.push_back(s.a);
        e->ev_pool.push_back(s.b);
    }
    e->spans.clear();
    return KDB_OK;
}

int ensure_staging(kdb_engine *e)
{
    if (e->staging_ready) return KDB_OK;
    for (int b = 0; b < NBUF; b++) {
        HIP_TRY(hipHostMalloc((void **)&e->h_bases[b], e->stage_bytes + 64, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **)&e->h_offs[b], (e->stage_reads + 1) * sizeof(uint64_t), hipHostMallocDefault));
        HIP_TRY(hipMalloc((void **)&e->d_bases[b], e->stage_bytes + 64));
        HIP_TRY(hipMalloc((void **)&e->d_offs[b], (e->stage_reads + 1) * sizeof(uint64_t)));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_copied[b], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_done[b], hipEventDisableTiming));
    }
    e->staging_ready = true;
    // (from k = 13 on every batch pays a sweep of the 4^k vector -- 0.5 GiB at k = 13 -- or, on the two-level path, partial pages of
    //  512 rings x 512 workgroups: 64 MiB chunks are appended on the device and counted 1 GiB at a time)
    const int64_t want = e->accum_bytes >= 0 ? e->accum_bytes : (e->k >= 13 ? (int64_t)1 << 30 : 0);
    if (want > 0) {
        e->acc_cap = (size_t)want < e->stage_bytes ? e->stage_bytes : (size_t)want;
        e->acc_reads_cap = e->acc_cap / 64 + e->stage_reads;
        for (int s = 0; s < 2; s++) {
            HIP_TRY(hipMalloc((void **)&e->d_acc_bases[s], e->acc_cap + 64));
            HIP_TRY(hipMalloc((void **)&e->d_acc_offs[s], (e->acc_reads_cap + 1) * sizeof(uint64_t)));
            HIP_TRY(hipEventCreateWithFlags(&e->ev_acc_done[s], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&e->ev_acc_copied, hipEventDisableTiming));
        e->acc_ready = true;
    }
    return KDB_OK;
}

// a histogram pass of the overlapped one-level path may still be running on s_hist: whatever else is about to touch the vector on
// the compute stream waits for it
int overlap_join(kdb_engine *e)
{
    if (e->ov.last < 0) return KDB_OK;
    HIP_TRY(hipStreamWaitEvent(e->s_compute, e->ov.hist_done[e->ov.last], 0));
    e->ov.last = -1;
    return KDB_OK;
}

// (re)create the compute stream and the histogram stream for the "overlap" options; nothing may be in flight
int overlap_streams(kdb_engine *e)
{
    const bool want_hist = e->overlap != 0, want_mask = want_hist && e->overlap_hist_cus > 0;
    if (e->s_hist) { HIP_TRY(hipStreamSynchronize(e->s_hist)); HIP_TRY(hipStreamDestroy(e->s_hist)); e->s_hist = nullptr; }
    kdb::overlap_free(e->ov);
    if (e->compute_masked || want_mask) {
        HIP_TRY(hipStreamSynchronize(e->s_compute));
        HIP_TRY(hipStreamDestroy(e->s_compute));
        e->s_compute = nullptr;
        e->compute_masked = false;
    }
    if (!want_hist) {
        if (!e->s_compute) HIP_TRY(hipStreamCreateWithFlags(&e->s_compute, hipStreamNonBlocking));
        return KDB_OK;
    }
    if (!want_mask) {
        if (!e->s_compute) HIP_TRY(hipStreamCreateWithFlags(&e->s_compute, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&e->s_hist, hipStreamNonBlocking));
        e->ov.grid = 0;
        return KDB_OK;
    }
    // Diagnostic only.  On ROCm 7.2 a process that has created a CU-masked stream crashes or hangs inside the runtime when a LATER hipMalloc
    // runs out of memory (tools/experiments/repro_r05_oom_after_cumask.py: torch filling the device after such an engine was closed) --
    // and the partition does not pay anyway.  Masks are therefore only made when the environment asks for them.
    if (!getenv("KDB_ALLOW_CU_MASKS")) {
        e->overlap_hist_cus = 0;
        (void)overlap_streams(e);
        return fail(KDB_ERR_ARG, "overlap_hist_cus: CU-masked streams are a diagnostic (set KDB_ALLOW_CU_MASKS=1; see include/kdbhip.h)");
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, e->device));
    const int ncu = prop.multiProcessorCount, H = e->overlap_hist_cus;
    if (H >= ncu || ncu > 1024) return fail(KDB_ERR_ARG, "overlap_hist_cus=%d of %d CUs", H, ncu);
    std::vector<uint32_t> mh((size_t)(ncu + 31) / 32, 0u), ms((size_t)(ncu + 31) / 32, 0u);
    int given = 0;
    for (int i = 0; i < ncu; i++) {
        bool hist;
        if (e->overlap_mask_mode == 1) hist = given < H && (int)(((long long)i * H) / ncu) != (int)(((long long)(i + 1) * H) / ncu);
        else if (e->overlap_mask_mode == 2) hist = given < H && (i % 32) < (H * 32 + ncu - 1) / ncu;
        else hist = i < H;
        if (hist) { mh[(size_t)i / 32] |= 1u << (i % 32); given++; } else ms[(size_t)i / 32] |= 1u << (i % 32);
    }
    HIP_TRY(hipExtStreamCreateWithCUMask(&e->s_compute, (uint32_t)ms.size(), ms.data()));
    e->compute_masked = true;
    HIP_TRY(hipExtStreamCreateWithCUMask(&e->s_hist, (uint32_t)mh.size(), mh.data()));
    e->ov.grid = 2u * (uint32_t)(ncu - given);                 // two persistent scatter workgroups per CU of the compute stream
    return KDB_OK;
}

enum : int { BATCH_HOST_FED = 1, BATCH_CONST_INPUT = 2 };
int grow(void **p, size_t *cap, size_t need_bytes);
int launch_batch(kdb_engine *e, uint8_t *d_bases, size_t nbytes, const uint64_t *d_offs, size_t nreads, int first_is_continuation, int flags);

// count what has been accumulated so far as one batch
int flush_accumulated(kdb_engine *e)
{
    if (!e->acc_ready || e->acc_nr == 0) return KDB_OK;
    const int s = e->acc_slot;
    HIP_TRY(hipEventRecord(e->ev_acc_copied, e->s_copy));
    HIP_TRY(hipStreamWaitEvent(e->s_compute, e->ev_acc_copied, 0));
    int rc = launch_batch(e, e->d_acc_bases[s], e->acc_nb, e->d_acc_offs[s], e->acc_nr, 0, BATCH_HOST_FED);
    if (rc != KDB_OK) return rc;
    HIP_TRY(hipEventRecord(e->ev_acc_done[s], e->s_compute));
    e->acc_inflight[s] = true;
    e->acc_slot = s ^ 1;
    e->acc_nb = e->acc_nr = 0;
    return KDB_OK;
}

// the staging vector of forward counts, allocated and zeroed at its first use.  No room for it: the batch in hand is counted canonically
// into d_table as without it (not an oom_fallback: no scratch was refused), and the next batch asks again.
bool ensure_fwd(kdb_engine *e)
{
    if (e->d_fwd) return true;
    if (hipMalloc((void **)&e->d_fwd, e->nbins * 8ull) != hipSuccess) { (void)hipGetLastError(); e->d_fwd = nullptr; return false; }
    if (hipMemsetAsync(e->d_fwd, 0, e->nbins * 8ull, e->s_compute) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(e->d_fwd); e->d_fwd = nullptr; return false; }
    return true;
}

// add the staged forward counts to the vector at the canonical bins and clear them; on s_compute, after everything that wrote d_fwd
int merge_strands(kdb_engine *e)
{
    if (!e->strands_pending) return KDB_OK;
    {
        ProfScope ps(e, KDB_KERNEL_STRAND_MERGE);
        kdbstrands::strand_merge_launch(e->s_compute, e->d_fwd, e->d_table, e->k);
    }
    e->strands_pending = false;
    HIP_TRY(hipGetLastError());
    return KDB_OK;
}

// launch the counting kernels over one device-resident batch, on s_compute
int launch_batch(kdb_engine *e, uint8_t *d_bases, size_t nbytes, const uint64_t *d_offs, size_t nreads, int first_is_continuation, int flags)
{
    if (nreads == 0) return KDB_OK;
    if (e->tableless) return fail(KDB_ERR_STATE, "this engine was created by kdb_create_ids: it has no count vector");
    const uint64_t ntiles = (nbytes + kdb::TILE_BYTES - 1) / kdb::TILE_BYTES;
    if (ntiles > 0x7FFFFFFFull) return fail(KDB_ERR_ARG, "batch too large: %zu bytes", nbytes);       // (before anything is written into the caller's buffer)
    // The LDS-histogram paths take a ragged batch's record starts from the offsets (lens_kernel fills first_rec; nothing is written
    // into the residues).  Only the direct-atomics kernel (algo 1, or the fallback when the scatter scratch does not fit) and the
    // old k <= 7 kernel still mark record starts as bit 7 of a record's first byte: the marks go on right before such a kernel and
    // come off again right after it -- also when this function gives up half way.
    bool marked = false;
    auto mark = [&]() {
        ProfScope ps(e, KDB_KERNEL_MARK);
        const unsigned mg = (unsigned)std::min<uint64_t>((nreads + 255) / 256, 4096);
        if (flags & BATCH_CONST_INPUT)          // the caller's buffer is never written: these kernels then need records of one length
            hipLaunchKernelGGL(kdb::require_uniform_kernel, dim3(1), dim3(1), 0, e->s_compute, e->d_ctr);
        else {
            hipLaunchKernelGGL(kdb::mark_reads_kernel, dim3(mg), dim3(256), 0, e->s_compute, d_bases, d_offs, (uint64_t)nreads,
                               first_is_continuation, e->d_ctr);          // (grid-stride: a uniform batch returns at once)
            marked = true;
        }
    };
    auto unmark = [&]() {
        if (!marked) return;
        ProfScope ps(e, KDB_KERNEL_MARK);
        const unsigned ug = (unsigned)std::min<uint64_t>((nreads + 255) / 256, 4096);
        hipLaunchKernelGGL(kdb::unmark_reads_kernel, dim3(ug), dim3(256), 0, e->s_compute, d_bases, d_offs, (uint64_t)nreads, first_is_continuation,
                           (const kdb::DevCounters *)e->d_ctr);
        marked = false;
    };
    bool no_first_rec = false;
    {
        // first_rec: one entry per 4 KiB of residues (grow-only scratch).  The batch before this one may still be reading the old array
        // (submits of device-resident input are asynchronous): drain the stream before it is freed.  No room for a larger one: the
        // direct-atomics kernel needs none, the batch is counted there (as when the scatter scratch does not fit).
        const size_t need = ((nbytes >> kdb::FIRST_REC_SHIFT) + 2) * sizeof(uint32_t);
        if (e->first_rec_cap < need && e->d_first_rec) HIP_TRY(hipStreamSynchronize(e->s_compute));
        int grc = grow((void **)&e->d_first_rec, &e->first_rec_cap, need);
        if (grc == KDB_ERR_NOMEM) no_first_rec = true;
        else if (grc != KDB_OK) return grc;
    }
    {
        ProfScope ps(e, KDB_KERNEL_MARK);
        const dim3 grid((unsigned)((nreads + 255) / 256)), block(256);
        // only the per-batch words: n_short, n_bad, bad_layout, not_uniform stay set until kdb_reset
        HIP_TRY(hipMemsetAsync(&e->d_ctr->neg_min_len, 0, kdb::PER_BATCH_WORDS * sizeof(unsigned long long), e->s_compute));
        const dim3 lgrid(grid.x < 1024u ? grid.x : 1024u);
        hipLaunchKernelGGL(kdb::lens_kernel, lgrid, block, 0, e->s_compute, d_offs, (uint64_t)nreads, (uint64_t)nbytes,
                           e->min_len > 0 ? e->min_len : e->k, first_is_continuation, e->d_ctr, e->d_first_rec);
        // bytes with bit 7 set are no residues (kmer.py:170 raises).  No pass of its own looks for them: the counting kernels'
        // front end counts them as bad; where the direct-atomics kernel runs over a ragged batch (its start marks are bit 7),
        // mark_reads_kernel reports a record start that carries the bit already, and any other such byte is a mark too many
        // (marks_seen != marks_set at the sync).  Host-fed and device-resident input alike.
    }
    if (nbytes == 0) return KDB_OK;          // only zero-length records: all short reads
    if (nreads > 0xFFFFFFF0ull) return fail(KDB_ERR_ARG, "batch of %zu records: at most 2^32 - 16 per submit", nreads);
    e->bytes_in += nbytes;
    const kdb::RecStarts rs{d_offs, e->d_first_rec, (uint32_t)nreads, first_is_continuation ? 1u : 0u};
    int algo = (int)e->algo;
    if (algo == 0 || algo == 3) algo = 2;                    // LDS-histogram paths unless told otherwise (3: the paged scatter's old number)
    if (no_first_rec && algo == 2) { algo = 1; e->oom_fallbacks++; e->tp.table_is_zero = false; }
    const bool paged2 = algo == 2 && e->k > e->opt.one_level_max_k;
    // only the deferred two-level flush may treat the vector as still all zero; everything else adds to it right away
    if (!paged2 || e->n_mode == KDB_N_EXPAND || !e->opt.defer) e->tp.table_is_zero = false;
    // a canonical batch of the one-level paths counts forward ids into the staging vector; the strands are merged at the sync
    const bool staged = e->canonical && e->strand_merge && algo == 2 && e->k <= std::min((int)e->opt.one_level_max_k, e->strand_merge_max_k) &&
                        !e->overlap && !e->smallk_old && ensure_fwd(e);
    const int canonical = staged ? 0 : e->canonical;
    unsigned long long *const table = staged ? e->d_fwd : e->d_table;
    if (staged) e->strands_pending = true;
    if (algo == 2) {
        EngineProf hook(e);
        const bool ex = e->n_mode == KDB_N_EXPAND;
        const kdb::ScBatch batch{d_bases, nbytes, rs, e->k, canonical, ex, table, e->d_ctr};
        int rc;
        if (e->k <= kdb::SMALLK_LDS_MAX_K && !e->smallk_old)
            rc = kdb::smallk_lds_count(e->s_compute, d_bases, nbytes, rs, e->k, canonical, ex, e->opt.grid, table, e->d_ctr, hook);
        else if (e->k <= kdb::SMALLK_MAX) {
            mark();
            rc = kdb::smallk_count(e->s_compute, d_bases, nbytes, e->k, canonical, ex, table, e->d_ctr, hook);
            unmark();
        }
        else if (e->k <= e->opt.one_level_max_k) {
            rc = 3;
            if (e->overlap && e->s_hist && !ex) rc = kdb::scatter_count_overlapped(e->ov, e->opt, e->s_compute, e->s_hist, batch, hook);
            if (rc == 3) {
                { const int jrc = overlap_join(e); if (jrc != KDB_OK) return jrc; }
                // (one_level_defer: stage 2 waits for more batches; 3 = no room for an arena of two regions, and nothing is pending)
                if (kdb::one_level_depth(e->opt, e->k) >= 2 && !(e->overlap && e->s_hist)) rc = kdb::scatter_count_deferred(e->ol, e->opt, e->s_compute, batch, hook);
                if (rc == 3) rc = kdb::scatter_count(e->sc, e->opt, e->s_compute, batch, hook);
            }
        }
        else {
            const size_t lost = nreads * (size_t)(e->k - 1);
            rc = kdb::twolevel_paged_count(e->tp, e->opt, e->s_compute, batch, nbytes > lost ? nbytes - lost : 0, hook);
        }
        if (rc == 2) { e->oom_fallbacks++; algo = 1; e->tp.table_is_zero = false; }   // no room for the scatter scratch: count this batch with direct atomics
        else if (rc != 0) return fail(KDB_ERR_HIP, "LDS-histogram path failed: %s", kdb::partition_error());
    }
    if (algo == 1) {
        { const int jrc = overlap_join(e); if (jrc != KDB_OK) return jrc; }
        mark();
        {
            ProfScope ps(e, KDB_KERNEL_COUNT);
            const bool ex = (e->n_mode == KDB_N_EXPAND);
            const dim3 grid((unsigned)ntiles), block(kdb::TPB);
#define KDB_LAUNCH_DIRECT(ID, EX)                                                                              \
    hipLaunchKernelGGL((kdb::count_direct_kernel<ID, EX>), grid, block, 0, e->s_compute, d_bases, (uint64_t)nbytes, \
                       e->k, canonical, table, e->d_ctr)
            if (e->k <= 16) { if (ex) KDB_LAUNCH_DIRECT(uint32_t, true); else KDB_LAUNCH_DIRECT(uint32_t, false); }
            else            { if (ex) KDB_LAUNCH_DIRECT(uint64_t, true); else KDB_LAUNCH_DIRECT(uint64_t, false); }
#undef KDB_LAUNCH_DIRECT
        }
        unmark();
    }
    if (e->n_mode == KDB_N_EXPAND && e->d_worklist) {
        ProfScope ps(e, KDB_KERNEL_COUNT);
        hipLaunchKernelGGL(kdb::expand_worklist_kernel, dim3(1024), dim3(256), 0, e->s_compute, table, e->d_ctr, e->k, canonical);
    }
    if (e->n_mode == KDB_N_DROP) {
        // residues that are neither ACGT nor N: an IUPAC code is only an error in a window that no N shields (kmer.py:287-289)
        ProfScope ps(e, KDB_KERNEL_MARK);
        hipLaunchKernelGGL(kdb::resolve_suspects_kernel, dim3(4), dim3(256), 0, e->s_compute, (const uint8_t *)d_bases, (uint64_t)nbytes, d_offs, (uint64_t)nreads,
                           e->k, e->d_ctr);
    }
    HIP_TRY(hipGetLastError());
    return KDB_OK;
}

// batches the two-level path, or the one-level path with one_level_defer, has scattered into a page arena but not yet added to the vector
int flush_pending_paged(kdb_engine *e)
{
    if (e->ol.used) {
        EngineProf hook(e);
        if (kdb::one_level_flush(e->ol, e->s_compute, e->d_ctr, hook)) return fail(KDB_ERR_HIP, "LDS-histogram path failed: %s", kdb::partition_error());
    }
    if (e->tp.pending == 0) return KDB_OK;
    EngineProf hook(e);
    if (kdb::twolevel_paged_flush(e->tp, e->opt, e->s_compute, e->d_table, e->d_ctr, hook)) return fail(KDB_ERR_HIP, "LDS-histogram path failed: %s", kdb::partition_error());
    return KDB_OK;
}

int check_errors(kdb_engine *e)
{
    kdb::DevCounters c;
    HIP_TRY(hipMemcpy(&c, e->d_ctr, sizeof c, hipMemcpyDeviceToHost));
    if (c.n_short)
        return fail(KDB_ERR_SHORT_READ, "%llu record(s) shorter than k=%d (reference: kmer.py:461-463 raises)",
                    c.n_short, e->k);
    if (c.bad_layout)
        return fail(KDB_ERR_ARG, "read_offsets must rise from 0 to nbytes (records tile the residue buffer exactly)");
    if (c.internal_err) {
        // Besides the page sequences (and the level-2 kernel's checks) a side list of the overlapped path raises this counter when it takes more pairs than
        // it has room for (hot_add).  Where a list's header still shows that -- it is written anew when a later batch uses the list -- say so: the
        // lists are sized from their batches (scatter_count_overlapped), so it means that the bound there is wrong, not that the input is.
        for (int q = 0; q < 2; q++) {
            unsigned long long hd[2] = {0, 0};
            if (e->ov.side[q] && hipMemcpy(hd, e->ov.side[q], sizeof hd, hipMemcpyDeviceToHost) == hipSuccess && hd[0] > hd[1])
                return fail(KDB_ERR_STATE, "internal: the overlapped path's side list of degenerate ids overflowed (%llu pairs for %llu places); counts are incomplete",
                            hd[0], hd[1]);
        }
        return fail(KDB_ERR_STATE, "internal: a scatter kernel ran out of its page sequence (%llu times); counts are incomplete", c.internal_err);
    }
    if (c.not_uniform)
        return fail(KDB_ERR_ARG, "kdb_submit_device_const needs records of one length (the buffer is never marked); use kdb_submit_device");
    if (c.n_bad)
        return fail(KDB_ERR_BAD_RESIDUE, "%llu residue(s) outside ACGTN%s (reference: kmer.py:309 / :170 raises)", c.n_bad,
                    e->n_mode == KDB_N_DROP ? " that no N in their window shields" : "");
    if (c.marks_seen != c.marks_set)
        return fail(KDB_ERR_BAD_RESIDUE, "the residue buffer holds %lld byte(s) with bit 7 set that are not record starts of their batch "
                                         "(not residues -- kmer.py:170 raises -- or marks left in a device buffer by a job that was aborted)",
                    (long long)(c.marks_seen - c.marks_set));
    return KDB_OK;
}

int grow(void **p, size_t *cap, size_t need_bytes)
{
    if (*cap >= need_bytes) return KDB_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    size_t want = need_bytes + need_bytes / 4 + 256;
    hipError_t err = hipMalloc(p, want);
    if (err != hipSuccess) { (void)hipGetLastError(); return fail(KDB_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(err)); }
    *cap = want;
    return KDB_OK;
}

// scratch of kdb_shred / kdb_window_ids: kept across calls (three hipMalloc + hipFree per record otherwise)
int shred_scratch(kdb_engine *e, size_t nbytes, size_t nreads)
{
    int rc;
    if ((rc = grow((void **)&e->sh_seq, &e->sh_seq_cap, nbytes + 64)) != KDB_OK) return rc;
    if ((rc = grow((void **)&e->sh_ids, &e->sh_ids_cap, nbytes * 8ull)) != KDB_OK) return rc;
    if (nreads && (rc = grow((void **)&e->sh_offs, &e->sh_offs_cap, (nreads + 1) * sizeof(uint64_t))) != KDB_OK) return rc;
    if (!e->sh_ctr) HIP_TRY(hipMalloc((void **)&e->sh_ctr, sizeof(kdb::DevCounters)));
    if (!e->sh_suspects) HIP_TRY(hipMalloc((void **)&e->sh_suspects, e->suspects_cap * sizeof(unsigned long long)));
    return KDB_OK;
}

int create_common(kdb_engine *e, kdb_engine **out)
{
    hipError_t err;
    if ((err = hipStreamCreateWithFlags(&e->s_compute, hipStreamNonBlocking)) != hipSuccess ||
        (err = hipStreamCreateWithFlags(&e->s_copy, hipStreamNonBlocking)) != hipSuccess ||
        (err = hipMalloc((void **)&e->d_ctr, sizeof(kdb::DevCounters))) != hipSuccess) {
        kdb_destroy(e);
        return fail(KDB_ERR_HIP, "engine setup failed: %s", hipGetErrorString(err));
    }
    int rc = kdb_reset(e);
    if (rc != KDB_OK) { kdb_destroy(e); return rc; }
    // KDB_ENGINE_OPTS="name=value,name=value": tuning options for every engine of the process (experiments and the test suite under an
    // option: tools/experiments/); an unknown name or a refused value fails the creation -- loudly, like kdb_set_option itself
    if (const char *opts = getenv("KDB_ENGINE_OPTS")) {
        std::string all(opts);
        for (size_t at = 0; at < all.size();) {
            size_t end = all.find(',', at);
            if (end == std::string::npos) end = all.size();
            const std::string kv = all.substr(at, end - at);
            at = end + 1;
            if (kv.empty()) continue;
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { kdb_destroy(e); return fail(KDB_ERR_ARG, "KDB_ENGINE_OPTS: '%s' is not name=value", kv.c_str()); }
            rc = kdb_set_option(e, kv.substr(0, eq).c_str(), (int64_t)strtoll(kv.c_str() + eq + 1, nullptr, 0));
            if (rc != KDB_OK) { kdb_destroy(e); return rc; }
        }
    }
    *out = e;
    return KDB_OK;
}

}  // namespace

// ---- the memory system's ceilings for the kernels' access patterns (diagnostic; bench.py) ----
namespace {
struct ProbePattern { const char *name; void (*launch)(const uint8_t *, uint64_t, uint8_t *, uint64_t, uint32_t, uint32_t *, hipStream_t); uint32_t read_bytes, write_bytes; };
template <int RM, int WM, int NR, int NW>
void probe_launch(const uint8_t *src, uint64_t sb, uint8_t *dst, uint64_t db, uint32_t steps, uint32_t *sink, hipStream_t st)
{
    hipLaunchKernelGGL((kdbprobe::pattern<RM, WM, NR, NW>), dim3(512), dim3(512), 0, st, src, sb, dst, db, steps, sink);
}
using namespace kdbprobe;
#define KDB_PROBE(name, RM, WM, NR, NW) {name, probe_launch<RM, WM, NR, NW>, (uint32_t)(NR * (RM == R_PAGES15 ? 1536 : RM ? 1024 : 0)), (uint32_t)(NW * (WM ? 1024 : 0))}
const ProbePattern PROBES[] = {
    KDB_PROBE("stream_read", R_STREAM, W_NONE, 4, 0),
    KDB_PROBE("stream_write", R_NONE, W_STREAM, 0, 4),
    KDB_PROBE("pages_1k_read", R_PAGES, W_NONE, 4, 0),                         // the histogram pass: whole 1 KiB pages, four in flight per wave
    KDB_PROBE("lines_64_write", R_NONE, W_LINES_SC1, 0, 2),                     // what rounds 2-4 wrote
    KDB_PROBE("pieces_128_write", R_NONE, W_CHUNK128_SC1, 0, 2),                // what round 5 writes
    KDB_PROBE("scatter_64", R_STREAM, W_LINES_SC1, 1, 2),                       // one-level scatter: 1 KiB of residues in per 2 KiB of elements out
    KDB_PROBE("scatter_128", R_STREAM, W_CHUNK128_SC1, 1, 2),
    KDB_PROBE("level1_64", R_STREAM, W_LINES_SC1, 1, 3),                        // level 1: 3 bytes out per residue
    KDB_PROBE("level1_128", R_STREAM, W_CHUNK128_SC1, 1, 3),
    KDB_PROBE("level2_64", R_PAGES15, W_LINES_SC1, 2, 2),                       // level 2: two 1.5 KiB pages in per 2 KiB out
    KDB_PROBE("level2_128", R_PAGES15, W_CHUNK128_SC1, 2, 2),
};
#undef KDB_PROBE
constexpr int N_PROBES = (int)(sizeof(PROBES) / sizeof(PROBES[0]));
}  // namespace

// ---- the engine's plain integer options (kdb_set_option / kdb_get_option): one row each; the odd ones are code in those two functions ----
namespace {
enum OptBefore { OPT_NOTHING, OPT_FLUSH_PENDING /* pending batches were scattered under the old value */, OPT_SYNC_AND_STREAMS /* kdb_sync, then overlap_streams */,
                 OPT_SYNC /* kdb_sync: staged strands are merged under the old value */, OPT_NO_STAGING /* refused once the staging buffers exist */ };
struct OptRow {
    const char *name;
    int64_t (*get)(kdb_engine *);
    void (*set)(kdb_engine *, int64_t) = nullptr;               // null: read-only
    bool boolean = false;                                       // stored as 0 / 1
    int64_t lo = INT64_MIN, hi = INT64_MAX;                     // what kdb_set_option accepts
    OptBefore before = OPT_NOTHING;                             // what must happen before the value changes
    const char *hint = "";                                      // the end of the message that refuses a value
    int64_t multiple_of = 1;
};
#define KDB_OPT_RO(field) [](kdb_engine *e) { return (int64_t)e->field; }
#define KDB_OPT(field) KDB_OPT_RO(field), [](kdb_engine *e, int64_t v) { e->field = (decltype(e->field))v; }
const OptRow OPTIONS[] = {
    {"algo", KDB_OPT(algo), false, 0, 3, OPT_NOTHING, " (0 auto, 1 direct atomics, 2 LDS-histogram paths)"},
    {"min_len", KDB_OPT(min_len), false, 0, 64},
    {"copy_threads", KDB_OPT(copy_threads), false, 1, 64},
    {"smallk_old", KDB_OPT(smallk_old), true},
    {"accum_bytes", KDB_OPT(accum_bytes), false, -1, INT64_MAX, OPT_NO_STAGING, " (-1 auto, 0 off, else bytes)"},
    {"stage_bytes", KDB_OPT(stage_bytes), false, 4096, INT64_MAX, OPT_NO_STAGING, " (>=4096, multiple of 16)", 16},
    {"stage_reads", KDB_OPT(stage_reads), false, 1, INT64_MAX, OPT_NO_STAGING},
    {"overlap", KDB_OPT(overlap), true, 0, 1024, OPT_SYNC_AND_STREAMS},
    {"overlap_hist_cus", KDB_OPT(overlap_hist_cus), false, 0, 1024, OPT_SYNC_AND_STREAMS},
    {"overlap_mask_mode", KDB_OPT(overlap_mask_mode), false, 0, 1024, OPT_SYNC_AND_STREAMS},
    {"strand_merge", KDB_OPT(strand_merge), true, 0, 1024, OPT_SYNC},
    {"strand_merge_max_k", KDB_OPT(strand_merge_max_k), false, 1, 17, OPT_SYNC, " (1..17; never more than one_level_max_k)"},
    // the paged paths' tuning (kdb::PagedOptions)
    {"sc_grid", KDB_OPT(opt.grid), false, 0, 1024, OPT_NOTHING, " (0..1024)"},
    // id = [ hi ][ bucket fields ][ lo ]: how many of a bucket's 15 (k = 17: 16) bin bits sit below the bucket field
    {"sc_lo_bits", KDB_OPT(opt.lo_bits), false, 0, kdb::SC_LO_BITS_MAX, OPT_FLUSH_PENDING, " (0 = the default of the path, 1..15)"},
    {"sc_contig_pages", KDB_OPT(opt.contig_pages), true},
    {"sc_wide_lines", KDB_OPT(opt.wide_lines), true},
    {"l1_wide_lines", KDB_OPT(opt.l1_wide), true},
    {"l2_wide_lines", KDB_OPT(opt.l2_wide), true},
    {"l1_one_round", KDB_OPT(opt.l1_one_round), true},
    {"l1_compiled_k", KDB_OPT(opt.l1k), true},
    {"one_level_max_k", KDB_OPT(opt.one_level_max_k), false, 12, kdb::SC1_K, OPT_FLUSH_PENDING, " (12 or 13)"},
    {"defer_flush", KDB_OPT(opt.defer), true},
    {"pending_budget", KDB_OPT(opt.budget_bytes), false, 0, INT64_MAX},
    {"reserve_bytes", KDB_OPT(opt.reserve_bytes), false, 0, INT64_MAX},
    {"arena_grow", KDB_OPT(opt.grow), false, 0, 2, OPT_NOTHING, " (0 never, 1 when it pays, 2 whenever the arena has filled up)"},
    {"arena_batches", KDB_OPT(opt.first_batches), false, 1, kdb::PAGED_PENDING_MAX, OPT_NOTHING, " (1..64: the arena's first size, in batches like the first one)"},
    {"one_level_defer", KDB_OPT(opt.one_level_defer), false, -1, kdb::PAGED_PENDING_MAX, OPT_FLUSH_PENDING,
     " (-1 = 4 for k <= 12 and 0 for k = 13, 0 = sort and histogram pass per batch, 2..64 = per that many batches)"},
    // what the engine reports
    {"k", KDB_OPT_RO(k)},
    {"arena_budget_bytes", [](kdb_engine *e) { return (int64_t)(e->opt.budget_bytes ? e->opt.budget_bytes : e->tp.budget_decided); }},
    {"free_at_sizing", KDB_OPT_RO(tp.free_at_sizing)},
    {"overlap_scatter_grid", KDB_OPT_RO(ov.grid)},
    {"oom_fallbacks", KDB_OPT_RO(oom_fallbacks)},
    {"pending_batches", KDB_OPT_RO(tp.pending)},
    {"one_level_pending", KDB_OPT_RO(ol.pending)},
    {"d2h_bytes", KDB_OPT_RO(d2h_bytes)},
    {"folded_files", KDB_OPT_RO(folded_files)},
    {"bytes_in", KDB_OPT_RO(bytes_in)},
    // (an engine has one k: it fills the two-level arena or the one-level path's, and these count whichever it is)
    {"arena_pages", [](kdb_engine *e) { return (int64_t)(e->tp.arena.cap + e->ol.arena.cap); }},
    {"arena_reallocs", [](kdb_engine *e) { return (int64_t)(e->tp.reallocs + e->ol.reallocs); }},
    {"hist_flushes", [](kdb_engine *e) { return (int64_t)(e->tp.flushes + e->ol.flushes); }},
    {"flushed_batches", [](kdb_engine *e) { return (int64_t)(e->tp.flushed_batches + e->ol.flushed_batches); }},
    {"full_flushes", [](kdb_engine *e) { return (int64_t)(e->tp.full_flushes + e->ol.full_flushes); }},
    {"arena_region_base", KDB_OPT_RO(ol.used)},                   // the page the next one-level region would begin at (0: nothing pending)
};
#undef KDB_OPT
#undef KDB_OPT_RO
static_assert(kdb::SC_LO_BITS_MAX == 15 && kdb::SC1_K == 13 && kdb::PAGED_PENDING_MAX == 64, "the hints of sc_lo_bits, one_level_max_k and arena_batches spell these out");

const OptRow *find_option(const char *name)
{
    for (const OptRow &row : OPTIONS) if (!strcmp(name, row.name)) return &row;
    return nullptr;
}
}  // namespace

// kdb_gram: the launch of one group of rows, by the sizes of its blocks
namespace {

struct GramGroup { uint32_t row0, nrows; int na, nb; bool diag; };

// the most workgroups per row of kdb_gram's and kdb_pairstats' sweeps (include/kdbhip.h)
uint32_t gram_grid_max(uint32_t nrows) { return nrows < KDB_GRAM_GRID_MANY_ROWS ? (uint32_t)KDB_GRAM_GRID_MAX : (uint32_t)KDB_GRAM_GRID_MAX_MANY_ROWS; }

void gram_launch(const GramGroup &gr, uint32_t gx, const unsigned long long *const *vecs, const kdbgram::Row *rows, uint32_t nchunks, uint32_t pstride, ulonglong2 *partials,
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

}  // namespace


extern "C" {

int kdb_abi_version(void) { return KDB_ABI_VERSION; }

const char *kdb_last_error(void) { return g_err.c_str(); }

int kdb_device_count(int *n_out)
{
    if (!n_out) return fail(KDB_ERR_ARG, "n_out is NULL");
    HIP_TRY(hipGetDeviceCount(n_out));
    return KDB_OK;
}

const char *kdb_prof_kernel_name(int kernel_id)
{
    if (kernel_id < 0 || kernel_id >= KDB_N_KERNELS) return "";
    return KERNEL_NAMES[kernel_id];
}

int kdb_create(int k, int canonicalize, int n_mode, int device_id, void *d_table, kdb_engine **out)
{
    if (!out) return fail(KDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (k < 1 || k > 17) return fail(KDB_ERR_ARG, "k=%d outside 1..17 (4^k uint64 table must fit in HBM)", k);
    if (n_mode != KDB_N_DROP && n_mode != KDB_N_EXPAND) return fail(KDB_ERR_ARG, "n_mode=%d", n_mode);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);
    kdb_engine *e = new kdb_engine();
    e->k = k; e->canonical = canonicalize ? 1 : 0; e->n_mode = n_mode; e->device = device_id;
    e->nbins = 1ull << (2 * k);
    if (d_table) {
        e->d_table = (unsigned long long *)d_table;
        e->owns_table = false;
    } else {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        const unsigned long long need = e->nbins * 8ull;
        if (free_b && need > free_b) {
            delete e;
            return fail(KDB_ERR_NOMEM, "4^%d uint64 table needs %llu bytes, device has %zu free", k, need, free_b);
        }
        hipError_t me = hipMalloc((void **)&e->d_table, need);
        if (me != hipSuccess) { delete e; return fail(KDB_ERR_NOMEM, "hipMalloc(%llu) failed: %s", need, hipGetErrorString(me)); }
        e->owns_table = true;
    }
    return create_common(e, out);
}

int kdb_create_ids(int k, int canonicalize, int device_id, kdb_engine **out)
{
    if (!out) return fail(KDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (k < 1 || k > 17) return fail(KDB_ERR_ARG, "k=%d outside 1..17", k);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);
    kdb_engine *e = new kdb_engine();
    e->k = k; e->canonical = canonicalize ? 1 : 0; e->n_mode = KDB_N_DROP; e->device = device_id;
    e->nbins = 0; e->tableless = true;
    return create_common(e, out);
}

int kdb_destroy(kdb_engine *e)
{
    if (!e) return KDB_OK;
    DeviceGuard g(e->device);
    if (e->s_compute) (void)hipStreamSynchronize(e->s_compute);
    if (e->s_copy) (void)hipStreamSynchronize(e->s_copy);
    if (e->s_hist) { (void)hipStreamSynchronize(e->s_hist); (void)hipStreamDestroy(e->s_hist); }
    kdb::overlap_free(e->ov);
    kdb::scatter_free(e->sc);
    kdb::twolevel_paged_free(e->tp);
    kdb::one_level_free(e->ol);
    for (auto &s : e->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    for (int b = 0; b < NBUF; b++) {
        if (e->h_bases[b]) (void)hipHostFree(e->h_bases[b]);
        if (e->h_offs[b]) (void)hipHostFree(e->h_offs[b]);
        if (e->d_bases[b]) (void)hipFree(e->d_bases[b]);
        if (e->d_offs[b]) (void)hipFree(e->d_offs[b]);
        if (e->ev_copied[b]) (void)hipEventDestroy(e->ev_copied[b]);
        if (e->ev_done[b]) (void)hipEventDestroy(e->ev_done[b]);
    }
    for (int s2 = 0; s2 < 2; s2++) {
        if (e->d_acc_bases[s2]) (void)hipFree(e->d_acc_bases[s2]);
        if (e->d_acc_offs[s2]) (void)hipFree(e->d_acc_offs[s2]);
        if (e->ev_acc_done[s2]) (void)hipEventDestroy(e->ev_acc_done[s2]);
    }
    if (e->ev_acc_copied) (void)hipEventDestroy(e->ev_acc_copied);
    for (int s2 = 0; s2 < 2; s2++) if (e->ev_pin[s2]) (void)hipEventDestroy(e->ev_pin[s2]);
    if (e->d_worklist) (void)hipFree(e->d_worklist);
    if (e->d_suspects) (void)hipFree(e->d_suspects);
    if (e->d_first_rec) (void)hipFree(e->d_first_rec);
    if (e->sh_suspects) (void)hipFree(e->sh_suspects);
    if (e->sh_seq) (void)hipFree(e->sh_seq);
    if (e->sh_offs) (void)hipFree(e->sh_offs);
    if (e->sh_ids) (void)hipFree(e->sh_ids);
    if (e->sh_ctr) (void)hipFree(e->sh_ctr);
    if (e->d_acc_table) (void)hipFree(e->d_acc_table);
    if (e->d_fwd) (void)hipFree(e->d_fwd);
    if (e->d_ctr) (void)hipFree(e->d_ctr);
    if (e->owns_table && e->d_table) (void)hipFree(e->d_table);
    if (e->s_compute) (void)hipStreamDestroy(e->s_compute);
    if (e->s_copy) (void)hipStreamDestroy(e->s_copy);
    delete e;
    return KDB_OK;
}

int kdb_reset(kdb_engine *e)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    DeviceGuard g(e->device);
    e->acc_nb = e->acc_nr = 0;                       // anything not yet counted is dropped with the vector
    kdb::twolevel_paged_drop(e->tp);
    kdb::one_level_drop(e->ol);
    HIP_TRY(hipStreamSynchronize(e->s_copy));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    if (e->s_hist) { HIP_TRY(hipStreamSynchronize(e->s_hist)); e->ov.last = -1; }
    if (e->nbins) HIP_TRY(hipMemsetAsync(e->d_table, 0, e->nbins * 8ull, e->s_compute));
    if (e->d_acc_table) HIP_TRY(hipMemsetAsync(e->d_acc_table, 0, e->nbins * 8ull, e->s_compute));
    if (e->strands_pending) { HIP_TRY(hipMemsetAsync(e->d_fwd, 0, e->nbins * 8ull, e->s_compute)); e->strands_pending = false; }   // (staged counts go with the vector)
    e->folded_files = e->folded_total = 0;
    e->tp.table_is_zero = e->owns_table && !e->table_escaped;             // (a caller-owned vector may be written by the caller at any time)
    HIP_TRY(hipMemsetAsync(e->d_ctr, 0, sizeof(kdb::DevCounters), e->s_compute));
    unsigned long long wl[2] = {0, 0}, sus[2] = {0, 0};
    if (e->n_mode == KDB_N_EXPAND) {
        if (!e->d_worklist) HIP_TRY(hipMalloc((void **)&e->d_worklist, e->worklist_cap * sizeof(unsigned long long)));
        wl[0] = (unsigned long long)(uintptr_t)e->d_worklist; wl[1] = (unsigned long long)e->worklist_cap;
        HIP_TRY(hipMemcpyAsync(&e->d_ctr->wl, wl, sizeof wl, hipMemcpyHostToDevice, e->s_compute));
    } else if (!e->tableless) {
        if (!e->d_suspects) HIP_TRY(hipMalloc((void **)&e->d_suspects, e->suspects_cap * sizeof(unsigned long long)));
        sus[0] = (unsigned long long)(uintptr_t)e->d_suspects; sus[1] = (unsigned long long)e->suspects_cap;
        HIP_TRY(hipMemcpyAsync(&e->d_ctr->sus, sus, sizeof sus, hipMemcpyHostToDevice, e->s_compute));
    }
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    return KDB_OK;
}

int kdb_submit_device(kdb_engine *e, void *d_bases, size_t nbytes, const void *d_read_offsets, size_t nreads)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (nreads && (!d_bases || !d_read_offsets)) return fail(KDB_ERR_ARG, "NULL device buffer");
    if (((uintptr_t)d_bases & 15u) != 0) return fail(KDB_ERR_ARG, "d_bases must be 16-byte aligned");
    DeviceGuard g(e->device);
    return launch_batch(e, (uint8_t *)d_bases, nbytes, (const uint64_t *)d_read_offsets, nreads, 0, 0);
}

int kdb_submit_device_const(kdb_engine *e, const void *d_bases, size_t nbytes, const void *d_read_offsets, size_t nreads)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (nreads && (!d_bases || !d_read_offsets)) return fail(KDB_ERR_ARG, "NULL device buffer");
    if (((uintptr_t)d_bases & 15u) != 0) return fail(KDB_ERR_ARG, "d_bases must be 16-byte aligned");
    DeviceGuard g(e->device);
    return launch_batch(e, (uint8_t *)const_cast<void *>(d_bases), nbytes, (const uint64_t *)d_read_offsets, nreads, 0, BATCH_CONST_INPUT);
}

static int submit_impl(kdb_engine *e, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads, bool src_pinned, bool first_continues = false)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (nreads == 0) return KDB_OK;
    if (!offs || (!bases && nbytes)) return fail(KDB_ERR_ARG, "NULL host buffer");
    if (offs[nreads] < offs[0] || offs[nreads] > nbytes) return fail(KDB_ERR_ARG, "read_offsets exceed nbytes");
    DeviceGuard g(e->device);
    int rc = ensure_staging(e);
    if (rc != KDB_OK) return rc;
    if (src_pinned) {
        const int pi = e->pin_idx;                 // holds the event of call N-2
        if (!e->ev_pin[pi]) HIP_TRY(hipEventCreateWithFlags(&e->ev_pin[pi], hipEventDisableTiming));
        if (e->pin_used[pi]) HIP_TRY(hipEventSynchronize(e->ev_pin[pi]));
    }
    const uint64_t cap = e->stage_bytes;
    const uint64_t overlap = (uint64_t)(e->k - 1);
    size_t r = 0;
    bool cont = first_continues;                 // the next piece continues a record split across buffers (or across calls)
    uint64_t carry = first_continues ? offs[0] : 0;     // where that piece starts
    while (r < nreads) {
        const int b = e->next_buf;
        if (e->inflight[b]) { HIP_TRY(hipEventSynchronize(e->busy[b])); e->inflight[b] = false; }
        uint8_t *hb = e->h_bases[b];
        uint64_t *ho = e->h_offs[b];
        const int first_is_cont = cont ? 1 : 0;
        const uint64_t start = cont ? carry : offs[r];
        // records are adjacent in `bases`: take the longest run of whole records that fits the buffer
        const size_t rmax = (nreads - r < e->stage_reads) ? nreads : r + e->stage_reads;
        const uint64_t *ub = std::upper_bound(offs + r + 1, offs + rmax + 1, start + cap);
        size_t r1 = (size_t)(ub - offs) - 1;            // offs[r1] <= start + cap
        uint64_t nb;
        size_t nr;
        ho[0] = 0;
        if (r1 <= r) {                                   // the record at r alone exceeds a buffer: tile it with k-1 overlap
            nb = cap; nr = 1; ho[1] = cap;
            carry = start + cap - overlap; cont = true;
        } else {
            nb = offs[r1] - start; nr = r1 - r;
            uint64_t prev = start;
            for (size_t i = 1; i <= nr; i++) {
                const uint64_t o = offs[r + i];
                if (o < prev) return fail(KDB_ERR_ARG, "read_offsets not monotone at %zu", r + i);
                prev = o;
                ho[i] = o - start;
            }
            r = r1; cont = false;
        }
        const bool accumulate = e->acc_ready && !first_is_cont && !cont && nb <= e->acc_cap && nr <= e->acc_reads_cap;
        if (accumulate) {
            if (e->acc_nb + nb > e->acc_cap || e->acc_nr + nr > e->acc_reads_cap) { rc = flush_accumulated(e); if (rc != KDB_OK) return rc; }
            const int s = e->acc_slot;
            if (e->acc_inflight[s]) { HIP_TRY(hipEventSynchronize(e->ev_acc_done[s])); e->acc_inflight[s] = false; }
            for (size_t i = 0; i <= nr; i++) ho[i] += e->acc_nb;                 // rebase onto the accumulated batch
            const uint8_t *src = src_pinned ? bases + start : hb;
            if (!src_pinned) parallel_copy(hb, bases + start, nb, e->copy_threads);
            HIP_TRY(hipMemcpyAsync(e->d_acc_bases[s] + e->acc_nb, src, nb, hipMemcpyHostToDevice, e->s_copy));
            // entries acc_nr .. acc_nr + nr of the offsets (entry acc_nr == acc_nb is rewritten with the same value)
            HIP_TRY(hipMemcpyAsync(e->d_acc_offs[s] + e->acc_nr, ho, (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->s_copy));
            HIP_TRY(hipEventRecord(e->ev_copied[b], e->s_copy));
            e->busy[b] = e->ev_copied[b];                                          // staging is free once the copies are done
            e->acc_nb += nb; e->acc_nr += nr;
        } else {
            rc = flush_accumulated(e);                                             // keep the two paths from interleaving on a buffer
            if (rc != KDB_OK) return rc;
            if (src_pinned) {
                HIP_TRY(hipMemcpyAsync(e->d_bases[b], bases + start, nb, hipMemcpyHostToDevice, e->s_copy));
            } else {
                parallel_copy(hb, bases + start, nb, e->copy_threads);
                HIP_TRY(hipMemcpyAsync(e->d_bases[b], hb, nb, hipMemcpyHostToDevice, e->s_copy));
            }
            HIP_TRY(hipMemcpyAsync(e->d_offs[b], ho, (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->s_copy));
            HIP_TRY(hipEventRecord(e->ev_copied[b], e->s_copy));
            HIP_TRY(hipStreamWaitEvent(e->s_compute, e->ev_copied[b], 0));
            rc = launch_batch(e, e->d_bases[b], nb, e->d_offs[b], nr, first_is_cont, BATCH_HOST_FED);
            if (rc != KDB_OK) return rc;
            HIP_TRY(hipEventRecord(e->ev_done[b], e->s_compute));
            e->busy[b] = e->ev_done[b];
        }
        e->inflight[b] = true;
        e->next_buf = (b + 1) % NBUF;
    }
    if (src_pinned) {
        HIP_TRY(hipEventRecord(e->ev_pin[e->pin_idx], e->s_copy));
        e->pin_used[e->pin_idx] = true;
        e->pin_idx ^= 1;
    }
    return KDB_OK;
}

int kdb_submit(kdb_engine *e, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads)
{
    return submit_impl(e, bases, nbytes, offs, nreads, false);
}

int kdb_submit_pinned(kdb_engine *e, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads)
{
    return submit_impl(e, bases, nbytes, offs, nreads, true);
}

int kdb_submit_ex(kdb_engine *e, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads, int flags)
{
    if (flags & ~(KDB_SUBMIT_PINNED | KDB_SUBMIT_CONTINUES)) return fail(KDB_ERR_ARG, "kdb_submit_ex: unknown flags 0x%x", flags);
    return submit_impl(e, bases, nbytes, offs, nreads, (flags & KDB_SUBMIT_PINNED) != 0, (flags & KDB_SUBMIT_CONTINUES) != 0);
}

int kdb_host_alloc(void **out, size_t nbytes)
{
    if (!out) return fail(KDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    hipError_t err = hipHostMalloc(out, nbytes ? nbytes : 1, hipHostMallocDefault);
    if (err != hipSuccess) return fail(KDB_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", nbytes, hipGetErrorString(err));
    return KDB_OK;
}

int kdb_host_free(void *p)
{
    if (p) HIP_TRY(hipHostFree(p));
    return KDB_OK;
}

int kdb_sync(kdb_engine *e)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    DeviceGuard g(e->device);
    { int rc = flush_accumulated(e); if (rc != KDB_OK) return rc; }
    { int rc = flush_pending_paged(e); if (rc != KDB_OK) return rc; }
    { int rc = merge_strands(e); if (rc != KDB_OK) return rc; }
    HIP_TRY(hipStreamSynchronize(e->s_copy));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    if (e->s_hist) { HIP_TRY(hipStreamSynchronize(e->s_hist)); e->ov.last = -1; }
    for (int b = 0; b < NBUF; b++) e->inflight[b] = false;
    e->acc_inflight[0] = e->acc_inflight[1] = false;
    if (e->prof) { int rc = prof_collect(e); if (rc != KDB_OK) return rc; }
#ifdef KDB_SC_PROF
    {
        unsigned long long h[32];
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(kdb::g_sc_prof), sizeof h) == hipSuccess && (h[8] || h[24])) {
            static const char *names[8] = {"ids", "requests+stage-next+writes", "barrier 1", "flush", "barrier 2", "drain", "flush: word, page turn, line list", "flush: list read, line read, store"};
            static const char *kern[2] = {"scatter_bases_kernel", "scatter_ids_kernel"};
            for (int s2 = 0; s2 < 2; s2++) {
                const unsigned long long *g = h + 16 * s2;
                if (!g[8]) continue;
                unsigned long long tot = 0;
                for (int q = 0; q < 8; q++) tot += g[q];
                fprintf(stderr, "[sc_prof] %s: %llu workgroups; wave-cycles by phase:", kern[s2], g[8]);
                for (int q = 0; q < 8; q++) fprintf(stderr, " %s %.1f%%", names[q], 100.0 * (double)g[q] / (double)tot);
                fprintf(stderr, " | total %.3g wave-cycles\n", (double)tot);
            }
            memset(h, 0, sizeof h);
            (void)hipMemcpyToSymbol(HIP_SYMBOL(kdb::g_sc_prof), h, sizeof h);
            // the last launch of each kernel: when its workgroups ended, relative to the launch's span (KDB_SC_WG_DUMP=file: every workgroup's)
            static unsigned long long wg[2][2][1024];
            if (hipMemcpyFromSymbol(wg, HIP_SYMBOL(kdb::g_sc_wg), sizeof wg) == hipSuccess) {
                for (int s2 = 0; s2 < 2; s2++) {
                    std::vector<unsigned long long> st, en;
                    for (int w = 0; w < 1024; w++) if (wg[s2][1][w]) { st.push_back(wg[s2][0][w]); en.push_back(wg[s2][1][w]); }
                    if (en.empty()) continue;
                    const unsigned long long t00 = *std::min_element(st.begin(), st.end()), t11 = *std::max_element(en.begin(), en.end());
                    if (const char *dump = getenv("KDB_SC_WG_DUMP")) {
                        if (FILE *f = fopen(dump, "a")) {
                            fprintf(f, "%s", kern[s2]);
                            for (size_t w = 0; w < en.size(); w++) fprintf(f, " %.4f", (double)(en[w] - t00) / (double)(t11 - t00));
                            fprintf(f, "\n");
                            fclose(f);
                        }
                    }
                    std::sort(en.begin(), en.end());
                    const double t0 = (double)t00, span = (double)t11 - t0;
                    fprintf(stderr, "[sc_prof] %s, last launch: %zu workgroups, %.0f us; ends at min %.1f%% p10 %.1f%% p50 %.1f%% p90 %.1f%% of it\n", kern[s2], en.size(), span / 100.0,
                            100.0 * ((double)en.front() - t0) / span, 100.0 * ((double)en[en.size() / 10] - t0) / span, 100.0 * ((double)en[en.size() / 2] - t0) / span,
                            100.0 * ((double)en[en.size() * 9 / 10] - t0) / span);
                }
                memset(wg, 0, sizeof wg);
                (void)hipMemcpyToSymbol(HIP_SYMBOL(kdb::g_sc_wg), wg, sizeof wg);
            }
        }
    }
#endif
    return check_errors(e);
}

// count_nonzero + Sum over `vec` (stats_kernel), optional copy to the host; leaves the results in *c
static int vector_stats(kdb_engine *e, const unsigned long long *vec, uint64_t *counts_out, kdb::DevCounters *c)
{
    HIP_TRY(hipMemsetAsync(&e->d_ctr->unique, 0, 2 * sizeof(unsigned long long), e->s_compute));
    {
        ProfScope ps(e, KDB_KERNEL_STATS);
        unsigned grid = (unsigned)((e->nbins + 255) / 256);
        if (grid > 256u * 16u) grid = 256u * 16u;
        hipLaunchKernelGGL(kdb::stats_kernel, dim3(grid), dim3(256), 0, e->s_compute, vec, e->nbins, e->d_ctr);
    }
    HIP_TRY(hipGetLastError());
    if (counts_out) {
        touch_pages(counts_out, e->nbins * 8ull, 2 * e->copy_threads);          // (while stats_kernel sweeps the vector)
        HIP_TRY(hipMemcpyAsync(counts_out, vec, e->nbins * 8ull, hipMemcpyDeviceToHost, e->s_compute));
        e->d2h_bytes += e->nbins * 8ull;
    }
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    if (e->prof) { int rc = prof_collect(e); if (rc != KDB_OK) return rc; }
    HIP_TRY(hipMemcpy(c, e->d_ctr, sizeof *c, hipMemcpyDeviceToHost));
    return KDB_OK;
}

int kdb_finish(kdb_engine *e, uint64_t *counts_out, uint64_t *total_kmers, uint64_t *unique_kmers)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (e->tableless) return fail(KDB_ERR_STATE, "this engine was created by kdb_create_ids: it has no count vector");
    DeviceGuard g(e->device);
    int rc = kdb_sync(e);
    if (rc != KDB_OK) return rc;
    kdb::DevCounters c;
    if ((rc = vector_stats(e, e->d_table, counts_out, &c)) != KDB_OK) return rc;
    if (c.sum != c.total_kmers)
        return fail(KDB_ERR_STATE, "internal: Sum(counts)=%llu but %llu k-mers were emitted", c.sum, c.total_kmers);
    if (total_kmers) *total_kmers = c.total_kmers;
    if (unique_kmers) *unique_kmers = c.unique;
    return KDB_OK;
}

int kdb_table_stats(kdb_engine *e, uint64_t *counts_out, uint64_t *sum_out, uint64_t *unique_out)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (e->tableless) return fail(KDB_ERR_STATE, "this engine was created by kdb_create_ids: it has no count vector");
    DeviceGuard g(e->device);
    int rc = kdb_sync(e);
    if (rc != KDB_OK) return rc;
    kdb::DevCounters c;
    if ((rc = vector_stats(e, e->d_table, counts_out, &c)) != KDB_OK) return rc;
    if (sum_out) *sum_out = c.sum;
    if (unique_out) *unique_out = c.unique;
    return KDB_OK;
}

int kdb_nullomers(kdb_engine *e, int folded, uint64_t *ids_out, uint64_t cap, uint64_t *n_out)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (e->tableless) return fail(KDB_ERR_STATE, "this engine was created by kdb_create_ids: it has no count vector");
    if (folded && !e->d_acc_table) return fail(KDB_ERR_STATE, "kdb_nullomers(folded) before any kdb_fold_file");
    DeviceGuard g(e->device);
    int rc = kdb_sync(e);
    if (rc != KDB_OK) return rc;
    const unsigned long long *vec = folded ? e->d_acc_table : e->d_table;
    if (((uintptr_t)vec & 15u) != 0) return fail(KDB_ERR_ARG, "the count vector must be 16-byte aligned for kdb_nullomers");
    const uint64_t ntiles = (e->nbins + kdb::NULL_TILE - 1) / kdb::NULL_TILE;
    const uint64_t nranges = (ntiles + kdb::NULL_RANGE_TILES - 1) / kdb::NULL_RANGE_TILES;
    struct Scratch {
        uint32_t *tile_counts = nullptr; unsigned long long *range_totals = nullptr, *out[2] = {nullptr, nullptr};
        hipEvent_t written[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
        ~Scratch()
        {
            (void)hipFree(tile_counts); (void)hipFree(range_totals);
            for (int b = 0; b < 2; b++) { (void)hipFree(out[b]); if (written[b]) (void)hipEventDestroy(written[b]); if (copied[b]) (void)hipEventDestroy(copied[b]); }
        }
    } sc;
    if (hipMalloc((void **)&sc.tile_counts, ntiles * sizeof(uint32_t)) != hipSuccess || hipMalloc((void **)&sc.range_totals, nranges * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_nullomers: no room for %llu tile counts", (unsigned long long)ntiles);
    }
    hipLaunchKernelGGL(kdb::null_count_kernel, dim3((unsigned)std::min<uint64_t>(ntiles, 256u * 16u)), dim3(kdb::NULL_TPB), 0, e->s_compute, vec, e->nbins, ntiles, sc.tile_counts);
    hipLaunchKernelGGL(kdb::null_scan_kernel, dim3((unsigned)nranges), dim3(1024), 0, e->s_compute, sc.tile_counts, ntiles, sc.range_totals);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> totals(nranges);
    HIP_TRY(hipMemcpyAsync(totals.data(), sc.range_totals, nranges * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->s_compute));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    uint64_t total = 0, largest = 0;
    for (uint64_t r = 0; r < nranges; r++) { total += totals[r]; largest = std::max<uint64_t>(largest, totals[r]); }
    if (n_out) *n_out = total;
    if (!ids_out || total == 0) return KDB_OK;
    if (total > cap) return fail(KDB_ERR_ARG, "kdb_nullomers: %llu ids do not fit the %llu entries given", (unsigned long long)total, (unsigned long long)cap);
    for (int b = 0; b < (nranges > 1 ? 2 : 1); b++) {
        if (hipMalloc((void **)&sc.out[b], largest * 8ull) != hipSuccess) { (void)hipGetLastError(); return fail(KDB_ERR_NOMEM, "kdb_nullomers: no room for %llu ids on the device", (unsigned long long)largest); }
        HIP_TRY(hipEventCreateWithFlags(&sc.written[b], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sc.copied[b], hipEventDisableTiming));
    }
    touch_pages(ids_out, total * 8ull, 2 * e->copy_threads);
    uint64_t at = 0;
    for (uint64_t r = 0; r < nranges; r++) {
        if (!totals[r]) continue;
        const int b = (int)(r & 1);
        const uint64_t tile0 = r * kdb::NULL_RANGE_TILES;
        const uint32_t here = (uint32_t)std::min<uint64_t>(kdb::NULL_RANGE_TILES, ntiles - tile0);
        HIP_TRY(hipStreamWaitEvent(e->s_compute, sc.copied[b], 0));                 // (the copy of range r - 2 has left this buffer; a no-op before the first record)
        hipLaunchKernelGGL(kdb::null_write_kernel, dim3(std::min<uint32_t>(here, 256u * 16u)), dim3(kdb::NULL_TPB), 0, e->s_compute, vec, e->nbins, tile0, here,
                           (const uint32_t *)sc.tile_counts, sc.out[b]);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(sc.written[b], e->s_compute));
        HIP_TRY(hipStreamWaitEvent(e->s_copy, sc.written[b], 0));
        HIP_TRY(hipMemcpyAsync(ids_out + at, sc.out[b], totals[r] * 8ull, hipMemcpyDeviceToHost, e->s_copy));
        HIP_TRY(hipEventRecord(sc.copied[b], e->s_copy));
        at += totals[r];
    }
    HIP_TRY(hipStreamSynchronize(e->s_copy));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    return KDB_OK;
}

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
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);

    // rows = pairs of blocks (bi <= bj), grouped by the kernel that serves them: the last block may hold fewer than B vectors
    const int nblk = (n + B - 1) / B, last = n - (nblk - 1) * B, nfull = last == B ? nblk : nblk - 1;
    std::vector<kdbgram::Row> rows;
    std::vector<GramGroup> groups;
    auto open_group = [&](int na, int nb, bool diag) { groups.push_back(GramGroup{(uint32_t)rows.size(), 0, na, nb, diag}); };
    auto close_group = [&]() { groups.back().nrows = (uint32_t)rows.size() - groups.back().row0; if (!groups.back().nrows) groups.pop_back(); };
    open_group(B, B, true);
    for (int b = 0; b < nfull; b++) rows.push_back(kdbgram::Row{(uint8_t)b, (uint8_t)b});
    close_group();
    open_group(B, B, false);
    for (int bi = 0; bi < nfull; bi++) for (int bj = bi + 1; bj < nfull; bj++) rows.push_back(kdbgram::Row{(uint8_t)bi, (uint8_t)bj});
    close_group();
    if (nfull < nblk) {
        open_group(last, last, true);
        rows.push_back(kdbgram::Row{(uint8_t)nfull, (uint8_t)nfull});
        close_group();
        open_group(B, last, false);
        for (int bi = 0; bi < nfull; bi++) rows.push_back(kdbgram::Row{(uint8_t)bi, (uint8_t)nfull});
        close_group();
    }
    const uint32_t nrows = (uint32_t)rows.size();
    // gram_kernel takes the whole chunks, gram_tail_kernel the bins behind them; a row's partials: one per workgroup, then the tail's
    const uint32_t nchunks = (uint32_t)(nbins / kdbgram::CHUNK_BINS), wg_chunks = kdbgram::TPB / 64;
    const uint32_t gx = std::max(1u, std::min((nchunks + wg_chunks - 1) / wg_chunks, gram_grid_max(nrows)));       // (any grid gives the same integers)
    const uint32_t nparts = gx + 1;
    struct Scratch {
        const unsigned long long **vecs = nullptr; kdbgram::Row *rows = nullptr; ulonglong2 *partials = nullptr, *out = nullptr;
        hipStream_t st = nullptr; hipEvent_t a = nullptr, b = nullptr;
        ~Scratch()
        {
            (void)hipFree(vecs); (void)hipFree(rows); (void)hipFree(partials); (void)hipFree(out);
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
            if (st) (void)hipStreamDestroy(st);
        }
    } sc;
    std::vector<const unsigned long long *> ptrs((size_t)nblk * B, (const unsigned long long *)d_vectors[0]);
    for (int i = 0; i < n; i++) ptrs[i] = (const unsigned long long *)d_vectors[i];
    if (hipMalloc((void **)&sc.vecs, ptrs.size() * sizeof(void *)) != hipSuccess || hipMalloc((void **)&sc.rows, nrows * sizeof(kdbgram::Row)) != hipSuccess ||
        hipMalloc((void **)&sc.partials, (uint64_t)nrows * nparts * NSLOT * sizeof(ulonglong2)) != hipSuccess ||
        hipMalloc((void **)&sc.out, (uint64_t)nrows * NSLOT * sizeof(ulonglong2)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_gram: no room for the partial sums of %u x %u workgroups", nrows, gx);
    }
    HIP_TRY(hipStreamCreateWithFlags(&sc.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&sc.a));
    HIP_TRY(hipEventCreate(&sc.b));
    HIP_TRY(hipMemcpyAsync(sc.vecs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemcpyAsync(sc.rows, rows.data(), nrows * sizeof(kdbgram::Row), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipEventRecord(sc.a, sc.st));
    for (const GramGroup &gr : groups) gram_launch(gr, gx, sc.vecs, sc.rows, nchunks, nparts, sc.partials, sc.st);
    hipLaunchKernelGGL(kdbgram::gram_tail_kernel, dim3(nrows), dim3(64), 0, sc.st, sc.vecs, (const kdbgram::Row *)sc.rows, n, (uint64_t)nchunks * kdbgram::CHUNK_BINS, nbins,
                       nparts, gx, sc.partials);
    hipLaunchKernelGGL(kdbgram::gram_combine_kernel, dim3(nrows), dim3(256), 0, sc.st, (const ulonglong2 *)sc.partials, nparts, sc.out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc.b, sc.st));
    std::vector<ulonglong2> res((size_t)nrows * NSLOT);
    HIP_TRY(hipMemcpyAsync(res.data(), sc.out, res.size() * sizeof(ulonglong2), hipMemcpyDeviceToHost, sc.st));
    HIP_TRY(hipStreamSynchronize(sc.st));
    if (kernel_ms_out) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc.a, sc.b));
        *kernel_ms_out = (double)ms;
    }
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
namespace {

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

struct PairGroup { uint32_t row0, nrows; int na, nb; bool diag; };

void pair_launch(const PairGroup &gr, uint32_t gx, const unsigned long long *const *vecs, const kdbpair::Row *rows, uint32_t nchunks, uint32_t pstride,
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

struct PairScratch {
    const unsigned long long **vecs = nullptr; void *rows = nullptr, *partials = nullptr, *out = nullptr; double *sums = nullptr;
    hipStream_t st = nullptr; hipEvent_t a = nullptr, b = nullptr;
    ~PairScratch()
    {
        (void)hipFree(vecs); (void)hipFree(rows); (void)hipFree(partials); (void)hipFree(out); (void)hipFree(sums);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        if (st) (void)hipStreamDestroy(st);
    }
};

}  // namespace

int kdb_pairstats(int device_id, const void *const *d_vectors, int n, uint64_t nbins, uint64_t *sums_out, uint64_t *nnz_out, uint64_t *l1_out,
                  uint64_t *linf_out, uint64_t *ne_out, uint64_t *both_out, double *kernel_ms_out)
{
    constexpr int B = kdbpair::B, HALF = kdbpair::HALF, NPAIR = kdbpair::NPAIR, PW = kdbpair::PAIR_WORDS, VW = kdbpair::VEC_WORDS, RW = kdbpair::ROW_WORDS;
    if (int rc = pair_check_args("kdb_pairstats", d_vectors, n, nbins)) return rc;
    if (!sums_out || !nnz_out || !l1_out || !linf_out || !ne_out || !both_out) return fail(KDB_ERR_ARG, "kdb_pairstats: the six output arrays must not be NULL");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);

    // rows, grouped by the kernel that serves them: the diagonal blocks (the last may hold fewer than B vectors), then every earlier block
    // against the later blocks' vectors, HALF at a time
    const int nblk = (n + B - 1) / B;
    auto block_size = [&](int b) { return std::min(B, n - b * B); };
    std::vector<kdbpair::Row> rows;
    std::vector<PairGroup> groups;
    auto push = [&](int a0, int na, int b0, int nb) {
        const bool diag = a0 == b0;
        if (groups.empty() || groups.back().na != na || groups.back().nb != nb || groups.back().diag != diag)
            groups.push_back(PairGroup{(uint32_t)rows.size(), 0, na, nb, diag});
        groups.back().nrows++;
        rows.push_back(kdbpair::Row{(uint8_t)a0, (uint8_t)na, (uint8_t)b0, (uint8_t)nb});
    };
    for (int b = 0; b < nblk; b++) push(b * B, block_size(b), b * B, block_size(b));
    for (int pass = 0; pass < 2; pass++)               // (rows of HALF vectors first, then the rows of a single one: two groups at most)
        for (int bj = 1; bj < nblk; bj++)
            for (int h = 0; h < block_size(bj); h += HALF) {
                const int nb = std::min(HALF, block_size(bj) - h);
                if ((nb == HALF) != (pass == 0)) continue;
                for (int bi = 0; bi < bj; bi++) push(bi * B, B, bj * B + h, nb);
            }
    const uint32_t nrows = (uint32_t)rows.size();
    // pair_kernel takes the whole chunks, pair_tail_kernel the bins behind them; a row's partials: one per workgroup, then the tail's
    const uint32_t nchunks = (uint32_t)(nbins / kdbpair::CHUNK_BINS), wg_chunks = kdbpair::TPB / 64;
    const uint32_t gx = std::max(1u, std::min((nchunks + wg_chunks - 1) / wg_chunks, gram_grid_max(nrows)));       // (any grid gives the same integers)
    const uint32_t nparts = gx + 1;
    PairScratch sc;
    std::vector<const unsigned long long *> ptrs((size_t)n);
    for (int i = 0; i < n; i++) ptrs[i] = (const unsigned long long *)d_vectors[i];
    if (hipMalloc((void **)&sc.vecs, ptrs.size() * sizeof(void *)) != hipSuccess || hipMalloc(&sc.rows, nrows * sizeof(kdbpair::Row)) != hipSuccess ||
        hipMalloc(&sc.partials, (uint64_t)nrows * nparts * RW * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&sc.out, (uint64_t)nrows * RW * sizeof(uint64_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_pairstats: no room for the partial records of %u x %u workgroups", nrows, gx);
    }
    HIP_TRY(hipStreamCreateWithFlags(&sc.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&sc.a));
    HIP_TRY(hipEventCreate(&sc.b));
    HIP_TRY(hipMemcpyAsync(sc.vecs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemcpyAsync(sc.rows, rows.data(), nrows * sizeof(kdbpair::Row), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipEventRecord(sc.a, sc.st));
    for (const PairGroup &gr : groups)
        pair_launch(gr, gx, sc.vecs, (const kdbpair::Row *)sc.rows, nchunks, nparts, (unsigned long long *)sc.partials, sc.st);
    hipLaunchKernelGGL(kdbpair::pair_tail_kernel, dim3(nrows), dim3(64), 0, sc.st, sc.vecs, (const kdbpair::Row *)sc.rows, (uint64_t)nchunks * kdbpair::CHUNK_BINS, nbins,
                       nparts, gx, (unsigned long long *)sc.partials);
    hipLaunchKernelGGL(kdbpair::pair_combine_kernel, dim3(nrows), dim3(256), 0, sc.st, (const unsigned long long *)sc.partials, nparts, (unsigned long long *)sc.out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc.b, sc.st));
    std::vector<unsigned long long> res((size_t)nrows * RW);
    HIP_TRY(hipMemcpyAsync(res.data(), sc.out, res.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, sc.st));
    HIP_TRY(hipStreamSynchronize(sc.st));
    if (kernel_ms_out) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc.a, sc.b));
        *kernel_ms_out = (double)ms;
    }
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
    DeviceGuard g(device_id);

    std::vector<kdbpair::FloatRow> rows;
    for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++) rows.push_back(kdbpair::FloatRow{(uint8_t)i, (uint8_t)j});
    const uint32_t nrows = (uint32_t)rows.size();
    const uint32_t nchunks = (uint32_t)(nbins / kdbpair::CHUNK_BINS), wg_chunks = kdbpair::TPB / 64;
    const uint32_t gx = std::max(1u, std::min((nchunks + wg_chunks - 1) / wg_chunks, (uint32_t)KDB_PAIRFLOAT_GRID_MAX));          // (a function of nbins alone: the order of the additions is fixed)
    const uint32_t nparts = gx + 1;
    PairScratch sc;
    std::vector<const unsigned long long *> ptrs((size_t)n);
    for (int i = 0; i < n; i++) ptrs[i] = (const unsigned long long *)d_vectors[i];
    if (hipMalloc((void **)&sc.vecs, ptrs.size() * sizeof(void *)) != hipSuccess || hipMalloc(&sc.rows, nrows * sizeof(kdbpair::FloatRow)) != hipSuccess ||
        hipMalloc((void **)&sc.sums, sums.size() * sizeof(double)) != hipSuccess ||
        hipMalloc(&sc.partials, (uint64_t)nrows * nparts * FW * sizeof(double)) != hipSuccess ||
        hipMalloc(&sc.out, (uint64_t)nrows * FW * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_pairfloat: no room for the partial sums of %u x %u workgroups", nrows, gx);
    }
    HIP_TRY(hipStreamCreateWithFlags(&sc.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&sc.a));
    HIP_TRY(hipEventCreate(&sc.b));
    HIP_TRY(hipMemcpyAsync(sc.vecs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemcpyAsync(sc.rows, rows.data(), nrows * sizeof(kdbpair::FloatRow), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemcpyAsync(sc.sums, sums.data(), sums.size() * sizeof(double), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipEventRecord(sc.a, sc.st));
    hipLaunchKernelGGL(kdbpair::pairfloat_kernel, dim3(gx, nrows), dim3(kdbpair::TPB), 0, sc.st, sc.vecs, (const kdbpair::FloatRow *)sc.rows, (const double *)sc.sums, nchunks,
                       nparts, (double *)sc.partials);
    hipLaunchKernelGGL(kdbpair::pairfloat_tail_kernel, dim3(nrows), dim3(64), 0, sc.st, sc.vecs, (const kdbpair::FloatRow *)sc.rows, (const double *)sc.sums,
                       (uint64_t)nchunks * kdbpair::CHUNK_BINS, nbins, nparts, gx, (double *)sc.partials);
    hipLaunchKernelGGL(kdbpair::pairfloat_combine_kernel, dim3(nrows), dim3(64), 0, sc.st, (const double *)sc.partials, nparts, (double *)sc.out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc.b, sc.st));
    std::vector<double> res((size_t)nrows * FW);
    HIP_TRY(hipMemcpyAsync(res.data(), sc.out, res.size() * sizeof(double), hipMemcpyDeviceToHost, sc.st));
    HIP_TRY(hipStreamSynchronize(sc.st));
    if (kernel_ms_out) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc.a, sc.b));
        *kernel_ms_out = (double)ms;
    }
    for (uint32_t r = 0; r < nrows; r++) {
        const size_t i = rows[r].i, j = rows[r].j;
        const bool empty = isums[2 * i] == 0 || isums[2 * j] == 0;
        canberra_out[i * n + j] = canberra_out[j * n + i] = res[(size_t)r * FW];
        js_out[i * n + j] = js_out[j * n + i] = empty ? (double)NAN : res[(size_t)r * FW + 1];
    }
    return KDB_OK;
}

// ---- median-of-ratios size factors and normalised counts (kdb_sizefactors.hip.h, kdb_select_host.cpp.h) ----
namespace {
struct SizeFactorScratch {
    const unsigned long long **vecs = nullptr; double *L = nullptr; unsigned long long *eligible = nullptr, *hist = nullptr; void *targets = nullptr;
    uint32_t *flag = nullptr;
    hipStream_t st = nullptr; hipEvent_t a = nullptr, b = nullptr;
    ~SizeFactorScratch()
    {
        (void)hipFree(vecs); (void)hipFree(L); (void)hipFree(eligible); (void)hipFree(hist); (void)hipFree(targets); (void)hipFree(flag);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        if (st) (void)hipStreamDestroy(st);
    }
};

uint32_t sizefactor_grid(uint64_t nbins)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nbins + kdbsf::WG_BINS - 1) / kdbsf::WG_BINS, kdbsf::MAX_GRID));
}
}  // namespace

int kdb_size_factors(int device_id, const void *const *d_vectors, int n, uint64_t nbins, double *log_sf_out, uint64_t *eligible_out, double *kernel_ms_out)
{
    constexpr int NB = kdbsf::NBUCKET;
    if (int rc = pair_check_args("kdb_size_factors", d_vectors, n, nbins)) return rc;
    if (!log_sf_out || !eligible_out) return fail(KDB_ERR_ARG, "kdb_size_factors: log_sf_out and eligible_out must not be NULL");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);

    SizeFactorScratch sc;
    std::vector<const unsigned long long *> ptrs((size_t)n);
    for (int i = 0; i < n; i++) ptrs[i] = (const unsigned long long *)d_vectors[i];
    const size_t hist_bytes = (size_t)n * 2 * NB * sizeof(uint64_t);
    if (hipMalloc((void **)&sc.L, ((nbins + 1) & ~1ull) * sizeof(double)) != hipSuccess || hipMalloc((void **)&sc.vecs, ptrs.size() * sizeof(void *)) != hipSuccess ||
        hipMalloc((void **)&sc.eligible, sizeof(uint64_t)) != hipSuccess || hipMalloc((void **)&sc.hist, hist_bytes) != hipSuccess ||
        hipMalloc(&sc.targets, (size_t)n * sizeof(kdbsf::Target)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_size_factors: no room for the float64 scratch of %llu bins", (unsigned long long)nbins);
    }
    HIP_TRY(hipStreamCreateWithFlags(&sc.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&sc.a));
    HIP_TRY(hipEventCreate(&sc.b));
    const uint32_t gx = sizefactor_grid(nbins);                                        // (any grid gives the same integers)
    double total_ms = 0.0;
    auto add_elapsed = [&]() -> hipError_t {
        float ms = 0;
        const hipError_t e = hipEventElapsedTime(&ms, sc.a, sc.b);
        total_ms += (double)ms;
        return e;
    };

    uint64_t m = 0;
    HIP_TRY(hipMemcpyAsync(sc.vecs, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemsetAsync(sc.eligible, 0, sizeof(uint64_t), sc.st));
    HIP_TRY(hipEventRecord(sc.a, sc.st));
    hipLaunchKernelGGL(kdbsf::geomean_kernel, dim3(gx), dim3(kdbsf::TPB), 0, sc.st, sc.vecs, n, nbins, sc.L, sc.eligible);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc.b, sc.st));
    HIP_TRY(hipMemcpyAsync(&m, sc.eligible, sizeof(uint64_t), hipMemcpyDeviceToHost, sc.st));
    HIP_TRY(hipStreamSynchronize(sc.st));
    HIP_TRY(add_elapsed());
    *eligible_out = m;
    if (kernel_ms_out) *kernel_ms_out = total_ms;
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
        HIP_TRY(hipMemcpyAsync(sc.targets, targets.data(), targets.size() * sizeof(kdbsf::Target), hipMemcpyHostToDevice, sc.st));
        HIP_TRY(hipMemsetAsync(sc.hist, 0, hist_bytes, sc.st));
        HIP_TRY(hipEventRecord(sc.a, sc.st));
        hipLaunchKernelGGL(kdbsf::select_kernel, dim3(gx, (uint32_t)n), dim3(kdbsf::TPB), 0, sc.st, sc.vecs, (const double *)sc.L, nbins,
                           (const kdbsf::Target *)sc.targets, kdbselect::pass_shift(pass), kdbselect::pass_width(pass), sc.hist);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(sc.b, sc.st));
        HIP_TRY(hipMemcpyAsync(hist.data(), sc.hist, hist_bytes, hipMemcpyDeviceToHost, sc.st));
        HIP_TRY(hipStreamSynchronize(sc.st));
        HIP_TRY(add_elapsed());
        for (int j = 0; j < n; j++)
            if (!sel[j].step(&hist[(size_t)j * 2 * NB], &hist[(size_t)j * 2 * NB + NB], pass))
                return fail(KDB_ERR_STATE, "kdb_size_factors: pass %d of the select found no element of the wanted rank in vector %d: the vectors changed during the call", pass, j);
    }
    for (int j = 0; j < n; j++) log_sf_out[j] = kdbselect::median_of(sel[j].low(), sel[j].high());
    if (kernel_ms_out) *kernel_ms_out = total_ms;
    return KDB_OK;
}

int kdb_scale_counts(int device_id, const void *d_vector, uint64_t nbins, double size_factor, void *d_out, int as_float64, double *kernel_ms_out)
{
    if (!d_vector || !d_out) return fail(KDB_ERR_ARG, "kdb_scale_counts: a vector is NULL");
    if ((((uintptr_t)d_vector | (uintptr_t)d_out) & 15u) != 0) return fail(KDB_ERR_ARG, "kdb_scale_counts: a vector is not 16-byte aligned");
    if (nbins == 0 || nbins > kdbsf::NBINS_MAX) return fail(KDB_ERR_ARG, "kdb_scale_counts: nbins is 0 or above 2^36 (64 x 4^17: more than a device holds)");
    if (!(size_factor > 0.0) || !std::isfinite(size_factor)) return fail(KDB_ERR_ARG, "kdb_scale_counts: the size factor %g is not finite and positive", size_factor);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);

    SizeFactorScratch sc;
    if (hipMalloc((void **)&sc.flag, sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_scale_counts: no room for the flag word");
    }
    HIP_TRY(hipStreamCreateWithFlags(&sc.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&sc.a));
    HIP_TRY(hipEventCreate(&sc.b));
    const uint32_t gx = sizefactor_grid(nbins);
    const unsigned long long *x = (const unsigned long long *)d_vector;
    uint32_t flag = 0;
    HIP_TRY(hipMemsetAsync(sc.flag, 0, sizeof(uint32_t), sc.st));
    HIP_TRY(hipEventRecord(sc.a, sc.st));
    // x < 2^64 rounds to at most 2^64: only a size factor of 2 or less can bring a quotient to 2^63.  Then a first sweep looks and writes
    // nothing, so that a refused call leaves d_out (which may be the input) as it was.
    if (!as_float64 && size_factor <= 2.0) {
        hipLaunchKernelGGL(kdbsf::scale_kernel, dim3(gx), dim3(kdbsf::TPB), 0, sc.st, x, nbins, size_factor, d_out, 0, 0, sc.flag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&flag, sc.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, sc.st));
        HIP_TRY(hipStreamSynchronize(sc.st));
        if (flag != 0) return fail(KDB_ERR_ARG, "kdb_scale_counts: a count divided by the size factor %g reaches 2^63: it has no place in an int64 matrix", size_factor);
    }
    hipLaunchKernelGGL(kdbsf::scale_kernel, dim3(gx), dim3(kdbsf::TPB), 0, sc.st, x, nbins, size_factor, d_out, as_float64 ? 1 : 0, 1, sc.flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc.b, sc.st));
    HIP_TRY(hipStreamSynchronize(sc.st));
    if (kernel_ms_out) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc.a, sc.b));
        *kernel_ms_out = (double)ms;
    }
    return KDB_OK;
}

// ---- abundance spectrum and doubled mid-ranks of a finished vector (kdb_spectrum.hip.h, kdb_spectrum_host.cpp.h) ----
namespace {
struct SpectrumScratch {
    unsigned long long *dense = nullptr;       // DENSE words, then the overflow list's counter
    unsigned long long *over = nullptr;        // `cap` values
    unsigned long long *tables = nullptr;      // kdb_rank_transform: the dense rank table, the distinct overflow values, their ranks
    uint64_t cap = 0;
    hipStream_t st = nullptr; hipEvent_t a = nullptr, b = nullptr;
    ~SpectrumScratch()
    {
        (void)hipFree(dense); (void)hipFree(over); (void)hipFree(tables);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        if (st) (void)hipStreamDestroy(st);
    }
};

// what both entry points check first; nothing on the device is touched
int spectrum_check_args(const char *who, int device_id, const void *d_vector, uint64_t nbins)
{
    if (!d_vector) return fail(KDB_ERR_ARG, "%s: the vector is NULL", who);
    if (((uintptr_t)d_vector & 15u) != 0) return fail(KDB_ERR_ARG, "%s: the vector is not 16-byte aligned", who);
    if (nbins == 0 || nbins > kdbspectrum::MAX_BINS) return fail(KDB_ERR_ARG, "%s: nbins is 0 or above 2^36 (64 x 4^17: more than a device holds)", who);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    return KDB_OK;
}

// (re)allocate the list for `cap` values; the table, the stream and the events at the first call
int spectrum_alloc(const char *who, SpectrumScratch &sc, uint64_t cap)
{
    if (!sc.dense && hipMalloc((void **)&sc.dense, (kdbspectrum::DENSE + 1) * 8ull) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "%s: no room for the table of %u multiplicities", who, kdbspectrum::DENSE);
    }
    (void)hipFree(sc.over);
    sc.over = nullptr;
    sc.cap = 0;
    if (cap && hipMalloc((void **)&sc.over, cap * 8ull) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "%s: no room for a list of %llu values of 65536 and above", who, (unsigned long long)cap);
    }
    sc.cap = cap;
    if (!sc.st) {
        HIP_TRY(hipStreamCreateWithFlags(&sc.st, hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&sc.a));
        HIP_TRY(hipEventCreate(&sc.b));
    }
    return KDB_OK;
}

// one sweep: host[0 .. DENSE) = the multiplicities, host[DENSE] = how many values the list would hold (sc.cap of them are stored); *ms += device time
int spectrum_sweep(SpectrumScratch &sc, const void *d_vector, uint64_t nbins, std::vector<uint64_t> &host, double *ms)
{
    const uint64_t nchunks = nbins / kdbspectrum::CHUNK_BINS;
    host.assign(kdbspectrum::DENSE + 1, 0);
    HIP_TRY(hipMemsetAsync(sc.dense, 0, (kdbspectrum::DENSE + 1) * 8ull, sc.st));
    HIP_TRY(hipEventRecord(sc.a, sc.st));
    hipLaunchKernelGGL(kdbspectrum::spectrum_kernel, dim3(kdbspectrum::spectrum_grid(nchunks)), dim3(kdbspectrum::TPB), 0, sc.st,
                       (const unsigned long long *)d_vector, nbins, nchunks, sc.dense, sc.over, (unsigned long long)sc.cap, sc.dense + kdbspectrum::DENSE);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc.b, sc.st));
    HIP_TRY(hipMemcpyAsync(host.data(), sc.dense, (kdbspectrum::DENSE + 1) * 8ull, hipMemcpyDeviceToHost, sc.st));
    HIP_TRY(hipStreamSynchronize(sc.st));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, sc.a, sc.b));
    *ms += (double)t;
    uint64_t total = host[kdbspectrum::DENSE];
    for (uint32_t v = 0; v < kdbspectrum::DENSE; v++) total += host[v];
    if (total != nbins) return fail(KDB_ERR_HIP, "the spectrum holds %llu bins, the vector %llu", (unsigned long long)total, (unsigned long long)nbins);
    return KDB_OK;
}
}  // namespace

int kdb_spectrum(int device_id, const void *d_vector, uint64_t nbins, uint64_t *dense_out, uint64_t *over_values_out, uint64_t over_cap,
                 uint64_t *n_over_out, double *kernel_ms_out)
{
    if (n_over_out) *n_over_out = 0;
    if (!dense_out || !n_over_out) return fail(KDB_ERR_ARG, "kdb_spectrum: dense_out and n_over_out must not be NULL");
    int rc = spectrum_check_args("kdb_spectrum", device_id, d_vector, nbins);
    if (rc != KDB_OK) return rc;
    DeviceGuard g(device_id);
    SpectrumScratch sc;
    if ((rc = spectrum_alloc("kdb_spectrum", sc, over_values_out ? std::min(over_cap, nbins) : 0)) != KDB_OK) return rc;
    std::vector<uint64_t> host;
    double ms = 0;
    if ((rc = spectrum_sweep(sc, d_vector, nbins, host, &ms)) != KDB_OK) return rc;
    const uint64_t n_over = host[kdbspectrum::DENSE];
    memcpy(dense_out, host.data(), kdbspectrum::DENSE * 8ull);
    *n_over_out = n_over;
    if (kernel_ms_out) *kernel_ms_out = ms;
    if (!over_values_out || n_over == 0) return KDB_OK;
    if (n_over > over_cap) return fail(KDB_ERR_ARG, "kdb_spectrum: %llu values of 65536 and above do not fit the %llu entries given", (unsigned long long)n_over, (unsigned long long)over_cap);
    HIP_TRY(hipMemcpy(over_values_out, sc.over, n_over * 8ull, hipMemcpyDeviceToHost));
    return KDB_OK;
}

int kdb_rank_transform(int device_id, const void *d_vector, uint64_t nbins, void *d_ranks_out, double *kernel_ms_out)
{
    if (nbins >= (1ull << 32)) return fail(KDB_ERR_ARG, "kdb_rank_transform: nbins is 2^32 or more (k >= 16): the doubled ranks sum to N (N + 1), which kdb_gram needs below 2^64");
    if (!d_ranks_out || ((uintptr_t)d_ranks_out & 15u) != 0) return fail(KDB_ERR_ARG, "kdb_rank_transform: the output is NULL or not 16-byte aligned");
    int rc = spectrum_check_args("kdb_rank_transform", device_id, d_vector, nbins);
    if (rc != KDB_OK) return rc;
    DeviceGuard g(device_id);
    SpectrumScratch sc;
    std::vector<uint64_t> host;
    double ms = 0;
    // the list is short on count profiles (at most Sum counts / 65536 values): a first guess, and a second sweep with the exact length where it was wrong
    if ((rc = spectrum_alloc("kdb_rank_transform", sc, std::min<uint64_t>(nbins, 1u << 20))) != KDB_OK) return rc;
    if ((rc = spectrum_sweep(sc, d_vector, nbins, host, &ms)) != KDB_OK) return rc;
    if (host[kdbspectrum::DENSE] > sc.cap) {
        if ((rc = spectrum_alloc("kdb_rank_transform", sc, host[kdbspectrum::DENSE])) != KDB_OK) return rc;
        if ((rc = spectrum_sweep(sc, d_vector, nbins, host, &ms)) != KDB_OK) return rc;
        if (host[kdbspectrum::DENSE] > sc.cap) return fail(KDB_ERR_STATE, "kdb_rank_transform: the vector changed during the call");
    }
    const uint64_t n_over = host[kdbspectrum::DENSE];
    std::vector<uint64_t> over(n_over);
    if (n_over) HIP_TRY(hipMemcpy(over.data(), sc.over, n_over * 8ull, hipMemcpyDeviceToHost));
    kdbspectrum_host::RankTables t;
    kdbspectrum_host::rank_tables(host.data(), kdbspectrum::DENSE, over.data(), n_over, t);
    if (t.nbins != nbins) return fail(KDB_ERR_HIP, "kdb_rank_transform: the rank tables cover %llu bins of %llu", (unsigned long long)t.nbins, (unsigned long long)nbins);
    const uint64_t nd = t.over_values.size();
    if (hipMalloc((void **)&sc.tables, (kdbspectrum::DENSE + 2 * nd) * 8ull) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_rank_transform: no room for the rank tables of %llu large values", (unsigned long long)nd);
    }
    HIP_TRY(hipMemcpyAsync(sc.tables, t.rank_dense.data(), kdbspectrum::DENSE * 8ull, hipMemcpyHostToDevice, sc.st));
    if (nd) {
        HIP_TRY(hipMemcpyAsync(sc.tables + kdbspectrum::DENSE, t.over_values.data(), nd * 8ull, hipMemcpyHostToDevice, sc.st));
        HIP_TRY(hipMemcpyAsync(sc.tables + kdbspectrum::DENSE + nd, t.over_ranks.data(), nd * 8ull, hipMemcpyHostToDevice, sc.st));
    }
    const kdbspectrum::RankTables dt{sc.tables, sc.tables + kdbspectrum::DENSE, sc.tables + kdbspectrum::DENSE + nd, (uint32_t)nd};
    const uint64_t nchunks = nbins / kdbspectrum::CHUNK_BINS;
    HIP_TRY(hipEventRecord(sc.a, sc.st));
    hipLaunchKernelGGL(kdbspectrum::rank_map_kernel, dim3(kdbspectrum::spectrum_grid(nchunks)), dim3(kdbspectrum::TPB), 0, sc.st,
                       (const unsigned long long *)d_vector, nbins, nchunks, dt, (unsigned long long *)d_ranks_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc.b, sc.st));
    HIP_TRY(hipStreamSynchronize(sc.st));
    float tm = 0;
    HIP_TRY(hipEventElapsedTime(&tm, sc.a, sc.b));
    if (kernel_ms_out) *kernel_ms_out = ms + (double)tm;
    return KDB_OK;
}

int kdb_strand_merge(int device_id, void *d_fwd, void *d_table, int k)
{
    if (k < 1 || k > 17) return fail(KDB_ERR_ARG, "kdb_strand_merge: k=%d outside 1..17", k);
    if (!d_fwd || !d_table || d_fwd == d_table) return fail(KDB_ERR_ARG, "kdb_strand_merge: d_fwd and d_table must be two vectors");
    if ((((uintptr_t)d_fwd | (uintptr_t)d_table) & 7u) != 0) return fail(KDB_ERR_ARG, "kdb_strand_merge: the vectors must be 8-byte aligned");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);
    struct Stream { hipStream_t st = nullptr; ~Stream() { if (st) (void)hipStreamDestroy(st); } } s;
    HIP_TRY(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
    kdbstrands::strand_merge_launch(s.st, (unsigned long long *)d_fwd, (unsigned long long *)d_table, k);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s.st));
    return KDB_OK;
}

int kdb_reduce(kdb_engine *const *engines, int n, int root)
{
    if (!engines || n < 2 || n > KDB_REDUCE_MAX) return fail(KDB_ERR_ARG, "kdb_reduce: n=%d engines (2..%d)", n, KDB_REDUCE_MAX);
    if (root < 0 || root >= n) return fail(KDB_ERR_ARG, "kdb_reduce: root=%d of %d", root, n);
    for (int j = 0; j < n; j++) {
        kdb_engine *e = engines[j];
        if (!e) return fail(KDB_ERR_ARG, "kdb_reduce: engine %d is NULL", j);
        if (e->tableless) return fail(KDB_ERR_STATE, "kdb_reduce: engine %d was created by kdb_create_ids: it has no count vector", j);
        if (e->k != engines[0]->k) return fail(KDB_ERR_ARG, "kdb_reduce: engine %d counts k=%d, engine 0 k=%d", j, e->k, engines[0]->k);
        if (((uintptr_t)e->d_table & 15u) != 0) return fail(KDB_ERR_ARG, "kdb_reduce: the count vector of engine %d is not 16-byte aligned", j);
        for (int i = 0; i < j; i++)
            if (engines[i] == e || engines[i]->d_table == e->d_table) return fail(KDB_ERR_ARG, "kdb_reduce: engines %d and %d are the same vector", i, j);
    }
    for (int j = 0; j < n; j++) { int rc = kdb_sync(engines[j]); if (rc != KDB_OK) return rc; }       // flushes what k >= 13 deferred
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) {
            const int dj = engines[j]->device, di = engines[i]->device;
            if (dj == di) continue;
            DeviceGuard g(dj);
            int can = 0;
            HIP_TRY(hipDeviceCanAccessPeer(&can, dj, di));
            if (!can) return fail(KDB_ERR_HIP, "kdb_reduce: device %d cannot access the memory of device %d", dj, di);
            const hipError_t pe = hipDeviceEnablePeerAccess(di, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
                return fail(KDB_ERR_HIP, "hipDeviceEnablePeerAccess(%d) on device %d failed: %s", di, dj, hipGetErrorString(pe));
            (void)hipGetLastError();
        }
    const uint64_t nbins = engines[0]->nbins;
    uint64_t bound[KDB_REDUCE_MAX + 1];
    for (int j = 0; j < n; j++) bound[j] = (nbins * (uint64_t)j / (uint64_t)n) & ~1ull;
    bound[n] = nbins;
    struct Events {
        hipEvent_t ev[KDB_REDUCE_MAX] = {nullptr}; int dev[KDB_REDUCE_MAX] = {0};
        ~Events() { for (int j = 0; j < KDB_REDUCE_MAX; j++) if (ev[j]) { DeviceGuard g(dev[j]); (void)hipEventDestroy(ev[j]); } }
    } evs;
    // every engine sums its slice of all the vectors
    for (int j = 0; j < n; j++) {
        kdb_engine *e = engines[j];
        if (bound[j + 1] <= bound[j]) continue;
        DeviceGuard g(e->device);
        kdb::ReducePeers peers;
        peers.n = 0;
        for (int i = 0; i < n; i++) if (i != j) peers.p[peers.n++] = engines[i]->d_table;
        const uint64_t pairs = (bound[j + 1] - bound[j] + 1) / 2;
        unsigned grid = (unsigned)std::min<uint64_t>((pairs + 255) / 256, 256u * 16u);
        hipLaunchKernelGGL(kdb::reduce_slice_kernel, dim3(grid), dim3(256), 0, e->s_compute, e->d_table, peers, bound[j], bound[j + 1]);
        HIP_TRY(hipGetLastError());
        evs.dev[j] = e->device;
        HIP_TRY(hipEventCreateWithFlags(&evs.ev[j], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(evs.ev[j], e->s_compute));
        e->tp.table_is_zero = false;
    }
    // the root collects the finished slices
    kdb_engine *r = engines[root];
    r->tp.table_is_zero = false;
    {
        DeviceGuard g(r->device);
        for (int j = 0; j < n; j++) {
            if (j == root || !evs.ev[j]) continue;
            kdb_engine *e = engines[j];
            const size_t bytes = (size_t)(bound[j + 1] - bound[j]) * 8u;
            HIP_TRY(hipStreamWaitEvent(r->s_compute, evs.ev[j], 0));
            if (e->device == r->device) HIP_TRY(hipMemcpyAsync(r->d_table + bound[j], e->d_table + bound[j], bytes, hipMemcpyDeviceToDevice, r->s_compute));
            else HIP_TRY(hipMemcpyPeerAsync(r->d_table + bound[j], r->device, e->d_table + bound[j], e->device, bytes, r->s_compute));
        }
        HIP_TRY(hipStreamSynchronize(r->s_compute));
    }
    // ... and now stands for all of them: Sum(counts) == k-mers emitted must hold for the root's kdb_finish
    unsigned long long total = 0;
    for (int j = 0; j < n; j++) {
        DeviceGuard g(engines[j]->device);
        unsigned long long t = 0;
        HIP_TRY(hipStreamSynchronize(engines[j]->s_compute));
        HIP_TRY(hipMemcpy(&t, &engines[j]->d_ctr->total_kmers, sizeof t, hipMemcpyDeviceToHost));
        total += t;
    }
    {
        DeviceGuard g(r->device);
        HIP_TRY(hipMemcpy(&r->d_ctr->total_kmers, &total, sizeof total, hipMemcpyHostToDevice));
    }
    return KDB_OK;
}

int kdb_fold_file(kdb_engine *e, uint64_t *total_kmers, uint64_t *unique_kmers) { return kdb_fold_file_into(e, e, total_kmers, unique_kmers); }

int kdb_fold_file_into(kdb_engine *e, kdb_engine *acc, uint64_t *total_kmers, uint64_t *unique_kmers)
{
    if (!e || !acc) return fail(KDB_ERR_ARG, "engine is NULL");
    if (e->tableless || acc->tableless) return fail(KDB_ERR_STATE, "this engine was created by kdb_create_ids: it has no count vector");
    if (e->k != acc->k || e->device != acc->device) return fail(KDB_ERR_ARG, "kdb_fold_file_into: the engines differ in k or device");
    DeviceGuard g(e->device);
    int rc = kdb_sync(e);
    if (rc != KDB_OK) return rc;
    if (((uintptr_t)e->d_table & 15u) != 0) return fail(KDB_ERR_ARG, "the count vector must be 16-byte aligned for kdb_fold_file");
    if (!acc->d_acc_table) {
        hipError_t me = hipMalloc((void **)&acc->d_acc_table, acc->nbins * 8ull);
        if (me != hipSuccess) { (void)hipGetLastError(); acc->d_acc_table = nullptr; return fail(KDB_ERR_NOMEM, "no room for a second 4^%d vector (accumulator): %s", e->k, hipGetErrorString(me)); }
        HIP_TRY(hipMemsetAsync(acc->d_acc_table, 0, acc->nbins * 8ull, e->s_compute));     // (ordered before this fold; later folds start after it has finished)
    }
    HIP_TRY(hipMemsetAsync(&e->d_ctr->unique, 0, 2 * sizeof(unsigned long long), e->s_compute));
    {
        ProfScope ps(e, KDB_KERNEL_STATS);
        unsigned grid = (unsigned)((e->nbins / 2 + 255) / 256);
        if (grid > 256u * 16u) grid = 256u * 16u;
        if (grid == 0) grid = 1;
        hipLaunchKernelGGL(kdb::fold_kernel, dim3(grid), dim3(256), 0, e->s_compute, e->d_table, acc->d_acc_table, e->nbins, e->d_ctr);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    if (e->prof) { rc = prof_collect(e); if (rc != KDB_OK) return rc; }
    kdb::DevCounters c;
    HIP_TRY(hipMemcpy(&c, e->d_ctr, sizeof c, hipMemcpyDeviceToHost));
    if (c.sum != c.total_kmers)
        return fail(KDB_ERR_STATE, "internal: Sum(counts)=%llu but %llu k-mers were emitted", c.sum, c.total_kmers);
    if (total_kmers) *total_kmers = c.total_kmers;
    if (unique_kmers) *unique_kmers = c.unique;
    acc->folded_files++;
    acc->folded_total += c.total_kmers;
    // the file vector is all zero again: a new file starts (what kdb_reset does, without a second sweep of the vector)
    HIP_TRY(hipMemsetAsync(&e->d_ctr->total_kmers, 0, sizeof(unsigned long long), e->s_compute));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    e->tp.table_is_zero = e->owns_table && !e->table_escaped;
    return KDB_OK;
}

int kdb_finish_folded(kdb_engine *e, uint64_t *counts_out, uint64_t *total_kmers, uint64_t *unique_kmers)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (!e->d_acc_table) return fail(KDB_ERR_STATE, "kdb_finish_folded before any kdb_fold_file");
    DeviceGuard g(e->device);
    int rc = kdb_sync(e);
    if (rc != KDB_OK) return rc;
    kdb::DevCounters c;
    if ((rc = vector_stats(e, e->d_acc_table, counts_out, &c)) != KDB_OK) return rc;
    if (c.sum != e->folded_total)
        return fail(KDB_ERR_STATE, "internal: Sum(accumulated counts)=%llu but the folded files held %llu k-mers", c.sum, (unsigned long long)e->folded_total);
    if (total_kmers) *total_kmers = c.sum;
    if (unique_kmers) *unique_kmers = c.unique;
    return KDB_OK;
}

int kdb_table(kdb_engine *e, void **d_table_out, uint64_t *nbins_out)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (d_table_out) { *d_table_out = e->d_table; e->table_escaped = true; e->tp.table_is_zero = false; }      // (the caller may write it from now on: RCCL reduces into it)
    if (nbins_out) *nbins_out = e->nbins;
    return KDB_OK;
}

int kdb_error_counts(kdb_engine *e, uint64_t *n_short, uint64_t *n_bad)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    DeviceGuard g(e->device);
    { int rc = flush_accumulated(e); if (rc != KDB_OK) return rc; }
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    kdb::DevCounters c;
    HIP_TRY(hipMemcpy(&c, e->d_ctr, sizeof c, hipMemcpyDeviceToHost));
    if (n_short) *n_short = c.n_short;
    if (n_bad) *n_bad = c.n_bad;
    return KDB_OK;
}

int kdb_shred(kdb_engine *e, const uint8_t *seq, size_t nbytes, uint64_t *ids_out, uint64_t *pos_out, size_t cap,
              size_t *n_out)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (n_out) *n_out = 0;
    if (!seq && nbytes) return fail(KDB_ERR_ARG, "seq is NULL");
    if (nbytes < (size_t)e->k)
        return fail(KDB_ERR_SHORT_READ, "record of %zu residues is shorter than k=%d (reference: kmer.py:461-463 raises)",
                    nbytes, e->k);
    if (nbytes > (1ull << 30)) return fail(KDB_ERR_ARG, "kdb_shred: at most 2^30 residues per call");
    DeviceGuard g(e->device);
    int rc = shred_scratch(e, nbytes, 0);
    if (rc != KDB_OK) return rc;
    std::vector<unsigned long long> ids(nbytes);
    kdb::DevCounters c;
    memset(&c, 0, sizeof c);
    const unsigned long long sus[2] = {(unsigned long long)(uintptr_t)e->sh_suspects, (unsigned long long)e->suspects_cap};
    HIP_TRY(hipMemcpyAsync(e->sh_seq, seq, nbytes, hipMemcpyHostToDevice, e->s_compute));
    HIP_TRY(hipMemsetAsync(e->sh_ctr, 0, sizeof c, e->s_compute));
    HIP_TRY(hipMemcpyAsync(&e->sh_ctr->sus, sus, sizeof sus, hipMemcpyHostToDevice, e->s_compute));
    hipLaunchKernelGGL(kdb::hibit_check_kernel, dim3(64), dim3(256), 0, e->s_compute, e->sh_seq, (uint64_t)nbytes, e->sh_ctr);
    const unsigned ntiles = (unsigned)((nbytes + kdb::TILE_BYTES - 1) / kdb::TILE_BYTES);
    hipLaunchKernelGGL(kdb::shred_kernel, dim3(ntiles), dim3(kdb::TPB), 0, e->s_compute, e->sh_seq, (uint64_t)nbytes, e->k,
                       e->canonical, e->sh_ids, e->sh_ctr);
    hipLaunchKernelGGL(kdb::resolve_suspects_kernel, dim3(1), dim3(256), 0, e->s_compute, (const uint8_t *)e->sh_seq, (uint64_t)nbytes, (const uint64_t *)nullptr,
                       (uint64_t)1, e->k, e->sh_ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ids.data(), e->sh_ids, nbytes * 8ull, hipMemcpyDeviceToHost, e->s_compute));
    HIP_TRY(hipMemcpyAsync(&c, e->sh_ctr, sizeof c, hipMemcpyDeviceToHost, e->s_compute));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    if (c.n_bad) return fail(KDB_ERR_BAD_RESIDUE, "%llu residue(s) outside ACGTN (reference: kmer.py:309 / :170 raises)", c.n_bad);
    size_t n = 0;
    for (size_t p = 0; p + (size_t)e->k <= nbytes; p++) {
        if (ids[p] == ~0ull) continue;
        if (n < cap) { if (ids_out) ids_out[n] = ids[p]; if (pos_out) pos_out[n] = p; }
        n++;
    }
    if (n_out) *n_out = n;
    return KDB_OK;
}

int kdb_window_ids(kdb_engine *e, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads, uint64_t *ids_out)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (nreads == 0 || nbytes == 0) return KDB_OK;
    if (!bases || !offs || !ids_out) return fail(KDB_ERR_ARG, "NULL buffer");
    if (offs[0] != 0 || offs[nreads] != nbytes) return fail(KDB_ERR_ARG, "read_offsets must start at 0 and end at nbytes");
    if (nbytes > (1ull << 30)) return fail(KDB_ERR_ARG, "kdb_window_ids: at most 2^30 residues per call");
    DeviceGuard g(e->device);
    int rc = shred_scratch(e, nbytes, nreads);
    if (rc != KDB_OK) return rc;
    kdb::DevCounters c;
    memset(&c, 0, sizeof c);
    HIP_TRY(hipMemcpyAsync(e->sh_seq, bases, nbytes, hipMemcpyHostToDevice, e->s_compute));
    HIP_TRY(hipMemcpyAsync(e->sh_offs, offs, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->s_compute));
    const unsigned long long sus[2] = {(unsigned long long)(uintptr_t)e->sh_suspects, (unsigned long long)e->suspects_cap};
    HIP_TRY(hipMemsetAsync(e->sh_ctr, 0, sizeof c, e->s_compute));
    HIP_TRY(hipMemcpyAsync(&e->sh_ctr->sus, sus, sizeof sus, hipMemcpyHostToDevice, e->s_compute));
    const dim3 grid((unsigned)((nreads + 255) / 256)), block(256), lgrid(grid.x < 1024u ? grid.x : 1024u);
    hipLaunchKernelGGL(kdb::lens_kernel, lgrid, block, 0, e->s_compute, e->sh_offs, (uint64_t)nreads, (uint64_t)nbytes,
                       e->min_len > 0 ? e->min_len : e->k, 0, e->sh_ctr, (uint32_t *)nullptr);
    hipLaunchKernelGGL(kdb::hibit_check_kernel, dim3(1024), dim3(256), 0, e->s_compute, e->sh_seq, (uint64_t)nbytes, e->sh_ctr);
    hipLaunchKernelGGL(kdb::mark_reads_kernel, dim3(grid.x < 4096u ? grid.x : 4096u), block, 0, e->s_compute, e->sh_seq, e->sh_offs, (uint64_t)nreads, 0,
                       e->sh_ctr);
    const unsigned ntiles = (unsigned)((nbytes + kdb::TILE_BYTES - 1) / kdb::TILE_BYTES);
    hipLaunchKernelGGL(kdb::shred_kernel, dim3(ntiles), dim3(kdb::TPB), 0, e->s_compute, e->sh_seq, (uint64_t)nbytes, e->k,
                       e->canonical, e->sh_ids, e->sh_ctr);
    hipLaunchKernelGGL(kdb::resolve_suspects_kernel, dim3(4), dim3(256), 0, e->s_compute, (const uint8_t *)e->sh_seq, (uint64_t)nbytes, (const uint64_t *)e->sh_offs,
                       (uint64_t)nreads, e->k, e->sh_ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ids_out, e->sh_ids, nbytes * 8ull, hipMemcpyDeviceToHost, e->s_compute));
    HIP_TRY(hipMemcpyAsync(&c, e->sh_ctr, sizeof c, hipMemcpyDeviceToHost, e->s_compute));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    if (c.bad_layout) return fail(KDB_ERR_ARG, "read_offsets must rise from 0 to nbytes");
    if (c.n_short) return fail(KDB_ERR_SHORT_READ, "%llu record(s) shorter than k=%d (reference: kmer.py:461-463 raises)", c.n_short, e->k);
    if (c.n_bad) return fail(KDB_ERR_BAD_RESIDUE, "%llu residue(s) outside ACGTN (reference: kmer.py:309 / :170 raises)", c.n_bad);
    return KDB_OK;
}

// ---- reads scored against a profile (kdb_score.hip.h) ----
namespace {
struct ScoreScratch {
    uint8_t *bases = nullptr; uint64_t *offs = nullptr; uint32_t *piece_rec = nullptr, *rec_piece0 = nullptr; kdbscore::PieceOut *pieces = nullptr;
    kdb::DevCounters *ctr = nullptr; double *log10_p = nullptr; unsigned long long *ints = nullptr;
    hipStream_t st = nullptr; hipEvent_t a = nullptr, b = nullptr;
    ~ScoreScratch()
    {
        (void)hipFree(bases); (void)hipFree(offs); (void)hipFree(piece_rec); (void)hipFree(rec_piece0); (void)hipFree(pieces); (void)hipFree(ctr);
        (void)hipFree(log10_p); (void)hipFree(ints);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        if (st) (void)hipStreamDestroy(st);
    }
};
}  // namespace

int kdb_score_reads(int device_id, const void *d_vector, int k, int canonical, uint64_t total, uint64_t pseudocount, const uint8_t *bases, size_t nbytes,
                    const uint64_t *offs, size_t nreads, int flags, double *log10_p_out, uint64_t *windows_out, uint64_t *zero_windows_out,
                    uint64_t *min_count_out, double *kernel_ms_out)
{
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (k < 1 || k > 17) return fail(KDB_ERR_ARG, "kdb_score_reads: k=%d out of range 1..17", k);
    if (!d_vector || ((uintptr_t)d_vector & 15u) != 0) return fail(KDB_ERR_ARG, "kdb_score_reads: the vector is NULL or not 16-byte aligned");
    if (flags & ~KDB_SCORE_CONTINUES) return fail(KDB_ERR_ARG, "kdb_score_reads: unknown flags %d", flags);
    if (total == 0) return fail(KDB_ERR_ARG, "kdb_score_reads: total is 0 (an empty profile gives no probabilities)");
    const uint64_t nbins = 1ull << (2 * k);
    const unsigned __int128 total2 = (unsigned __int128)total + (unsigned __int128)pseudocount * nbins;
    if ((total2 >> 64) != 0 || pseudocount >= (1ull << 62))
        return fail(KDB_ERR_ARG, "kdb_score_reads: total + pseudocount * 4^k and 4 * pseudocount must stay below 2^64");
    if (nreads == 0) return nbytes == 0 ? KDB_OK : fail(KDB_ERR_ARG, "kdb_score_reads: residues but no records");
    if (!offs || (!bases && nbytes) || !log10_p_out || !windows_out || !zero_windows_out || !min_count_out) return fail(KDB_ERR_ARG, "kdb_score_reads: NULL buffer");
    if (nbytes > (1ull << 30)) return fail(KDB_ERR_ARG, "kdb_score_reads: at most 2^30 residues per call");
    if (nreads > (1ull << 30)) return fail(KDB_ERR_ARG, "kdb_score_reads: at most 2^30 records per call");
    const bool continues = (flags & KDB_SCORE_CONTINUES) != 0;
    // the layout, and with it every address the kernels form, is settled here: the offsets are host memory
    if (offs[0] != 0 || offs[nreads] != nbytes) return fail(KDB_ERR_ARG, "read_offsets must start at 0 and end at nbytes");
    std::vector<uint32_t> rec_piece0(nreads + 1);
    uint64_t npieces = 0, nshort = 0;
    for (size_t r = 0; r < nreads; r++) {
        if (offs[r + 1] < offs[r] || offs[r + 1] > nbytes) return fail(KDB_ERR_ARG, "read_offsets must rise from 0 to nbytes");
        const uint64_t len = offs[r + 1] - offs[r];
        if (len < (uint64_t)k && !(r == 0 && continues)) nshort++;
        const uint64_t nwin = len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0;
        rec_piece0[r] = (uint32_t)npieces;
        npieces += std::max<uint64_t>(1, (nwin + kdbscore::PIECE - 1) / kdbscore::PIECE);         // (< 2^31: 2^30 records and 2^30 windows at most)
    }
    rec_piece0[nreads] = (uint32_t)npieces;
    if (nshort) return fail(KDB_ERR_SHORT_READ, "%llu record(s) shorter than k=%d (reference: kmer.py:461-463 raises)", (unsigned long long)nshort, k);
    std::vector<uint32_t> piece_rec;
    if (npieces != nreads) {
        piece_rec.resize(npieces);
        for (size_t r = 0; r < nreads; r++)
            for (uint32_t p = rec_piece0[r]; p < rec_piece0[r + 1]; p++) piece_rec[p] = (uint32_t)r;
    }
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);

    ScoreScratch sc;
    if (hipMalloc((void **)&sc.bases, ((nbytes + 15) & ~(size_t)15) + 32) != hipSuccess /* (piece_kernel's aligned words reach 23 bytes past a window's start) */ || hipMalloc((void **)&sc.offs, (nreads + 1) * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc((void **)&sc.rec_piece0, (nreads + 1) * sizeof(uint32_t)) != hipSuccess ||
        (!piece_rec.empty() && hipMalloc((void **)&sc.piece_rec, npieces * sizeof(uint32_t)) != hipSuccess) ||
        hipMalloc((void **)&sc.pieces, npieces * sizeof(kdbscore::PieceOut)) != hipSuccess || hipMalloc((void **)&sc.ctr, sizeof(kdb::DevCounters)) != hipSuccess ||
        hipMalloc((void **)&sc.log10_p, nreads * sizeof(double)) != hipSuccess || hipMalloc((void **)&sc.ints, 3 * nreads * sizeof(uint64_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_score_reads: no room for the scratch of %zu residues in %zu records", nbytes, nreads);
    }
    HIP_TRY(hipStreamCreateWithFlags(&sc.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&sc.a));
    HIP_TRY(hipEventCreate(&sc.b));
    kdb::DevCounters c;
    memset(&c, 0, sizeof c);
    c.sus_count = 1;                       // more than sus_cap = 0: resolve_suspects_kernel judges every residue of the batch itself
    if (nbytes) HIP_TRY(hipMemcpyAsync(sc.bases, bases, nbytes, hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemcpyAsync(sc.offs, offs, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemcpyAsync(sc.rec_piece0, rec_piece0.data(), (nreads + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, sc.st));
    if (!piece_rec.empty()) HIP_TRY(hipMemcpyAsync(sc.piece_rec, piece_rec.data(), npieces * sizeof(uint32_t), hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemcpyAsync(sc.ctr, &c, sizeof c, hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipEventRecord(sc.a, sc.st));
    // what kdb_window_ids refuses: bytes with bit 7 set, letters outside ACGTN that no N shields (kmer.py:309 / :170)
    hipLaunchKernelGGL(kdb::hibit_check_kernel, dim3(1024), dim3(256), 0, sc.st, (const uint8_t *)sc.bases, (uint64_t)nbytes, sc.ctr);
    const unsigned check_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(2048, (nbytes / 64 + 255) / 256));
    hipLaunchKernelGGL(kdb::resolve_suspects_kernel, dim3(check_grid), dim3(256), 0, sc.st, (const uint8_t *)sc.bases, (uint64_t)nbytes, (const uint64_t *)sc.offs,
                       (uint64_t)nreads, k, sc.ctr);
    unsigned long long *ints = sc.ints;
    hipLaunchKernelGGL(kdbscore::piece_kernel, dim3((unsigned)((npieces + kdbscore::TPB / 64 - 1) / (kdbscore::TPB / 64))), dim3(kdbscore::TPB), 0, sc.st,
                       (const uint8_t *)sc.bases, (const uint64_t *)sc.offs, (const uint32_t *)sc.piece_rec, (const uint32_t *)sc.rec_piece0, (uint32_t)npieces,
                       (const unsigned long long *)d_vector, k, canonical ? 1 : 0, (unsigned long long)pseudocount, sc.pieces);
    hipLaunchKernelGGL(kdbscore::record_kernel, dim3((unsigned)((nreads + 255) / 256)), dim3(256), 0, sc.st, (const kdbscore::PieceOut *)sc.pieces,
                       (const uint32_t *)sc.rec_piece0, (uint64_t)nreads, (double)(uint64_t)total2, continues ? 1 : 0, sc.log10_p, ints, ints + nreads, ints + 2 * nreads);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc.b, sc.st));
    HIP_TRY(hipMemcpyAsync(&c, sc.ctr, sizeof c, hipMemcpyDeviceToHost, sc.st));
    HIP_TRY(hipStreamSynchronize(sc.st));
    if (kernel_ms_out) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc.a, sc.b));
        *kernel_ms_out = (double)ms;
    }
    if (c.n_bad) return fail(KDB_ERR_BAD_RESIDUE, "%llu residue(s) outside ACGTN (reference: kmer.py:309 / :170 raises)", c.n_bad);
    HIP_TRY(hipMemcpy(log10_p_out, sc.log10_p, nreads * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(windows_out, ints, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(zero_windows_out, ints + nreads, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(min_count_out, ints + 2 * nreads, nreads * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return KDB_OK;
}

int kdb_parse_fastq(const uint8_t *text, size_t n, int at_eof, uint8_t *bases_out, size_t bases_cap, uint64_t *offsets_out,
                    size_t cap_reads, uint64_t *header_spans_out, size_t *nreads_out, size_t *nbases_out, size_t *consumed_out)
{
    if ((!text && n) || !bases_out || !offsets_out || !nreads_out || !nbases_out || !consumed_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    int rc = kdbhost::parse_fastq(text, n, at_eof, bases_out, bases_cap, offsets_out, cap_reads, header_spans_out, nreads_out,
                                  nbases_out, consumed_out, &why);
    if (rc) return fail(KDB_ERR_ARG, "kdb_parse_fastq: %s", why);
    return KDB_OK;
}

int kdb_parse_fastq_mt(const uint8_t *text, size_t n, int at_eof, uint8_t *bases_out, size_t bases_cap, uint64_t *offsets_out,
                       size_t cap_reads, uint64_t *header_spans_out, size_t *nreads_out, size_t *nbases_out, size_t *consumed_out, int nthreads)
{
    if ((!text && n) || !bases_out || !offsets_out || !nreads_out || !nbases_out || !consumed_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    int rc = kdbhost::parse_fastq_mt(text, n, at_eof, bases_out, bases_cap, offsets_out, cap_reads, header_spans_out, nreads_out,
                                     nbases_out, consumed_out, &why, nthreads);
    if (rc) return fail(KDB_ERR_ARG, "kdb_parse_fastq: %s", why);
    return KDB_OK;
}

int kdb_parse_fasta(const uint8_t *text, size_t n, uint8_t *bases_out, size_t bases_cap, uint64_t *offsets_out, size_t cap_reads,
                    uint64_t *header_spans_out, size_t *nreads_out, size_t *nbases_out)
{
    if ((!text && n) || !bases_out || !offsets_out || !nreads_out || !nbases_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    int rc = kdbhost::parse_fasta(text, n, bases_out, bases_cap, offsets_out, cap_reads, header_spans_out, nreads_out, nbases_out, &why);
    if (rc) return fail(KDB_ERR_ARG, "kdb_parse_fasta: %s", why);
    return KDB_OK;
}

int kdb_parse_fasta_chunk(const uint8_t *text, size_t n, int at_eof, int in_record, uint8_t *bases_out, size_t bases_cap, uint64_t *offsets_out,
                          size_t cap_reads, uint64_t *header_spans_out, size_t *nreads_out, size_t *nbases_out, size_t *consumed_out, int *in_record_out)
{
    if ((!text && n) || !bases_out || !offsets_out || !nreads_out || !nbases_out || !consumed_out || !in_record_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    int rc = kdbhost::parse_fasta_chunk(text, n, at_eof, in_record, bases_out, bases_cap, offsets_out, cap_reads, header_spans_out, nreads_out, nbases_out,
                                        consumed_out, in_record_out, &why);
    if (rc) return fail(KDB_ERR_ARG, "kdb_parse_fasta_chunk: %s", why);
    return KDB_OK;
}

int kdb_bgzf_inflate(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, int nthreads, size_t *consumed_out, size_t *produced_out)
{
    if ((!src && n) || !dst || !consumed_out || !produced_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    if (kdbhost::bgzf_inflate(src, n, dst, cap, nthreads, consumed_out, produced_out, &why)) return fail(KDB_ERR_ARG, "kdb_bgzf_inflate: %s", why);
    return KDB_OK;
}

int kdb_bgzf_scan(const char *path, uint64_t *coff_out, uint64_t *uoff_out, size_t cap, size_t *n_out)
{
    if (!path || !coff_out || !uoff_out || !n_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    const int rc = kdbhost::bgzf_scan(path, coff_out, uoff_out, cap, n_out, &why);
    if (rc == 2) return fail(KDB_ERR_NOMEM, "kdb_bgzf_scan('%s'): %s", path, why);
    if (rc) return fail(KDB_ERR_ARG, "kdb_bgzf_scan('%s'): %s", path, why);
    return KDB_OK;
}

struct kdb_gz { kdbhost::GzStream *s; };

int kdb_gz_open(const char *path, kdb_gz **out)
{
    if (!path || !out) return fail(KDB_ERR_ARG, "NULL argument");
    *out = nullptr;
    const char *why = "";
    kdbhost::GzStream *s = kdbhost::gz_open(path, &why);
    if (!s) return fail(KDB_ERR_ARG, "kdb_gz_open('%s'): %s", path, why);
    *out = new kdb_gz{s};
    return KDB_OK;
}

int kdb_gz_read(kdb_gz *g, uint8_t *dst, size_t cap, size_t *n_out)
{
    if (!g || (!dst && cap) || !n_out) return fail(KDB_ERR_ARG, "NULL argument");
    *n_out = 0;
    if (g->s->read(dst, cap, n_out)) return fail(KDB_ERR_ARG, "kdb_gz_read: %s", g->s->err.c_str());
    return KDB_OK;
}

int kdb_gz_close(kdb_gz *g)
{
    if (!g) return KDB_OK;
    delete g->s;
    delete g;
    return KDB_OK;
}

int kdb_write_kdb_rows_ex(const char *path, const uint64_t *counts, uint64_t nbins, uint64_t total_kmers, int compresslevel,
                          int nthreads, int encoder, uint64_t *nblocks_out)
{
    if (!path || (!counts && nbins)) return fail(KDB_ERR_ARG, "NULL argument");
    if (encoder != KDB_ENCODER_DEFAULT && encoder != KDB_ENCODER_ROWS && encoder != KDB_ENCODER_ZLIB)
        return fail(KDB_ERR_ARG, "kdb_write_kdb_rows: unknown encoder %d", encoder);
    if (compresslevel < 0 || compresslevel > 9) return fail(KDB_ERR_ARG, "kdb_write_kdb_rows: compresslevel %d (0..9)", compresslevel);
    const char *why = "";
    if (kdbhost::write_kdb_rows(path, counts, nbins, total_kmers, compresslevel, nthreads, nblocks_out, &why, encoder))
        return fail(KDB_ERR_ARG, "kdb_write_kdb_rows('%s'): %s", path, why);
    return KDB_OK;
}

int kdb_write_kdb_rows(const char *path, const uint64_t *counts, uint64_t nbins, uint64_t total_kmers, int compresslevel,
                       int nthreads, uint64_t *nblocks_out)
{
    return kdb_write_kdb_rows_ex(path, counts, nbins, total_kmers, compresslevel, nthreads, KDB_ENCODER_DEFAULT, nblocks_out);
}

int kdb_copy_back_and_write_kdb_rows(kdb_engine *e, int folded, uint64_t *counts_out, const char *path, uint64_t total_kmers, int compresslevel,
                                     int nthreads, int encoder, uint64_t *nblocks_out)
{
    if (!e || !counts_out || !path) return fail(KDB_ERR_ARG, "NULL argument");
    if (e->tableless) return fail(KDB_ERR_STATE, "this engine was created by kdb_create_ids: it has no count vector");
    if (folded && !e->d_acc_table) return fail(KDB_ERR_STATE, "kdb_copy_back_and_write_kdb_rows(folded) before any kdb_fold_file");
    if (encoder != KDB_ENCODER_DEFAULT && encoder != KDB_ENCODER_ROWS && encoder != KDB_ENCODER_ZLIB)
        return fail(KDB_ERR_ARG, "kdb_copy_back_and_write_kdb_rows: unknown encoder %d", encoder);
    DeviceGuard g(e->device);
    { int rc = kdb_sync(e); if (rc != KDB_OK) return rc; }
    const unsigned long long *vec = folded ? e->d_acc_table : e->d_table;
    const uint64_t nbins = e->nbins;
    touch_pages(counts_out, nbins * 8ull, 2 * e->copy_threads);
    // the vector comes back in pieces on a thread of its own; the writer's threads start on a chunk of rows as soon as it is there
    std::atomic<uint64_t> rows_ready{0};
    hipError_t copy_err = hipSuccess;
    const int device = e->device;
    std::thread copier([&] {
        if (hipSetDevice(device) != hipSuccess) { copy_err = hipErrorInvalidDevice; rows_ready.store(~0ull); return; }
        const uint64_t piece = (128ull << 20) / 8;
        for (uint64_t at = 0; at < nbins; at += piece) {
            const uint64_t n = std::min(piece, nbins - at);
            const hipError_t err = hipMemcpy(counts_out + at, vec + at, n * 8ull, hipMemcpyDeviceToHost);
            if (err != hipSuccess) { copy_err = err; rows_ready.store(~0ull); return; }
            rows_ready.store(at + n, std::memory_order_release);
        }
    });
    const char *why = "";
    const int wrc = kdbhost::write_kdb_rows(path, counts_out, nbins, total_kmers, compresslevel, nthreads, nblocks_out, &why, encoder, &rows_ready);
    copier.join();
    e->d2h_bytes += nbins * 8ull;
    if (copy_err != hipSuccess) return fail(KDB_ERR_HIP, "copying the count vector back failed: %s", hipGetErrorString(copy_err));
    if (wrc) return fail(KDB_ERR_ARG, "kdb_copy_back_and_write_kdb_rows('%s'): %s", path, why);
    return KDB_OK;
}

int kdb_read_kdb_rows(const char *path, uint64_t nbins, uint64_t *kmer_ids_out, uint64_t *counts_out, double *frequencies_out, int nthreads,
                      uint64_t *nrows_out)
{
    if (!path || !kmer_ids_out || !counts_out || !frequencies_out || !nrows_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    const int rc = kdbhost::read_kdb_rows(path, nbins, kmer_ids_out, counts_out, frequencies_out, nthreads, nrows_out, &why);
    if (rc == 3) return fail(KDB_ERR_STATE, "kdb_read_kdb_rows('%s'): not a file of BGZF members", path);
    if (rc) return fail(KDB_ERR_ARG, "kdb_read_kdb_rows('%s'): %s", path, why);
    return KDB_OK;
}

int kdb_format_frequency(uint64_t count, uint64_t total, char *buf, size_t cap)
{
    if (!buf || cap < 40) return fail(KDB_ERR_ARG, "buffer too small");
    int n = kdbhost::py_float_repr((double)count / (double)total, buf);
    buf[n] = 0;
    return KDB_OK;
}

int kdb_prof_enable(kdb_engine *e, int on)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    e->prof = on != 0;
    return KDB_OK;
}

int kdb_prof_reset(kdb_engine *e)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    DeviceGuard g(e->device);
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    int rc = prof_collect(e);
    if (rc != KDB_OK) return rc;
    for (int i = 0; i < KDB_N_KERNELS; i++) { e->prof_ms[i] = 0; e->prof_n[i] = 0; }
    return KDB_OK;
}

int kdb_prof_get(kdb_engine *e, int kernel_id, double *total_ms, uint64_t *launches)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (kernel_id < 0 || kernel_id >= KDB_N_KERNELS) return fail(KDB_ERR_ARG, "kernel_id=%d", kernel_id);
    DeviceGuard g(e->device);
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    int rc = prof_collect(e);
    if (rc != KDB_OK) return rc;
    if (total_ms) *total_ms = e->prof_ms[kernel_id];
    if (launches) *launches = e->prof_n[kernel_id];
    return KDB_OK;
}

// ---- the memory system's ceilings for the kernels' access patterns (diagnostic; bench.py): the table of patterns is above, before the C interface ----
int kdb_hbm_pattern_count(void) { return N_PROBES; }

const char *kdb_hbm_pattern_name(int i) { return (i >= 0 && i < N_PROBES) ? PROBES[i].name : ""; }

int kdb_hbm_pattern_probe(int device_id, double *gb_per_s_out, int n_out)
{
    if (!gb_per_s_out || n_out < N_PROBES) return fail(KDB_ERR_ARG, "kdb_hbm_pattern_probe: room for %d results needed", N_PROBES);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);
    const uint64_t region = 4ull << 30;                  // far beyond the 256 MB memory-side cache: every piece is written (read) once
    uint8_t *src = nullptr, *dst = nullptr; uint32_t *sink = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    int rc = KDB_OK;
    if (hipMalloc((void **)&src, region) != hipSuccess || hipMalloc((void **)&dst, region) != hipSuccess || hipMalloc((void **)&sink, 64) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(KDB_ERR_NOMEM, "kdb_hbm_pattern_probe: no room for two regions of 4 GiB");
    } else if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess ||
               hipMemsetAsync(src, 1, region, st) != hipSuccess || hipMemsetAsync(dst, 0, region, st) != hipSuccess) {
        rc = fail(KDB_ERR_HIP, "kdb_hbm_pattern_probe: setup failed");
    } else {
        for (int i = 0; i < N_PROBES && rc == KDB_OK; i++) {
            const uint64_t per_step = 512ull * 8ull * ((uint64_t)PROBES[i].read_bytes + PROBES[i].write_bytes);
            const uint32_t steps = (uint32_t)(6.0e9 / (double)per_step) + 1;
            float best = 1e30f;
            for (int rep = 0; rep < 3; rep++) {
                (void)hipEventRecord(a, st);
                PROBES[i].launch(src, region, dst, region, steps, sink, st);
                (void)hipEventRecord(b, st);
                if (hipEventSynchronize(b) != hipSuccess) { rc = fail(KDB_ERR_HIP, "kdb_hbm_pattern_probe: pattern '%s' failed", PROBES[i].name); break; }
                float ms = 0;
                (void)hipEventElapsedTime(&ms, a, b);
                if (rep && ms < best) best = ms;
            }
            gb_per_s_out[i] = (double)steps * (double)per_step / 1e6 / (double)best;
        }
    }
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (st) (void)hipStreamDestroy(st);
    if (src) (void)hipFree(src);
    if (dst) (void)hipFree(dst);
    if (sink) (void)hipFree(sink);
    return rc;
}

int kdb_set_option(kdb_engine *e, const char *name, int64_t value)
{
    if (!e || !name) return fail(KDB_ERR_ARG, "NULL argument");
    // (sc_top_bits=1 is the old name of sc_lo_bits=15: buckets from the leading id bits)
    if (!strcmp(name, "sc_top_bits")) return kdb_set_option(e, "sc_lo_bits", value ? kdb::SC_LO_BITS_MAX : 0);
#ifdef KDB_SC_PROF
    if (!strcmp(name, "sc_ablate")) { int v = (int)value; (void)hipMemcpyToSymbol(HIP_SYMBOL(kdb::g_sc_ablate), &v, sizeof v); return KDB_OK; }
#endif
    const OptRow *row = find_option(name);
    if (!row || !row->set) return fail(KDB_ERR_ARG, "unknown option '%s'", name);
    if (row->before == OPT_NO_STAGING && e->staging_ready) return fail(KDB_ERR_STATE, "staging already allocated");
    if (value < row->lo || value > row->hi || value % row->multiple_of) return fail(KDB_ERR_ARG, "%s=%lld%s", name, (long long)value, row->hint);
    // defer_flush = 0: what is pending is added to the vector now
    if (row->before == OPT_FLUSH_PENDING || (!strcmp(name, "defer_flush") && !value)) {
        DeviceGuard g(e->device);
        int rc = flush_pending_paged(e);
        if (rc != KDB_OK) return rc;
    }
    if (!strcmp(name, "pending_budget")) e->tp.budget_decided = e->ol.budget_decided = 0;      // (pending_budget = 0: the arena's size is decided anew at its next use)
    if (row->before != OPT_SYNC_AND_STREAMS && row->before != OPT_SYNC) { row->set(e, row->boolean ? (value ? 1 : 0) : value); return KDB_OK; }
    DeviceGuard g(e->device);
    { int rc = kdb_sync(e); if (rc != KDB_OK) return rc; }
    row->set(e, row->boolean ? (value ? 1 : 0) : value);
    return row->before == OPT_SYNC ? KDB_OK : overlap_streams(e);
}

int kdb_get_option(kdb_engine *e, const char *name, int64_t *value)
{
    if (!e || !name || !value) return fail(KDB_ERR_ARG, "NULL argument");
    if (const OptRow *row = find_option(name)) { *value = row->get(e); return KDB_OK; }
    if (!strcmp(name, "free_hbm")) {
        DeviceGuard g(e->device);
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        *value = (int64_t)free_b; return KDB_OK;
    }
    if (!strcmp(name, "arena_used_bound") || !strcmp(name, "arena_worst_case") || !strcmp(name, "arena_cursor")) {
        // pages of the arena the pending batches hold: the host's present bound (worst cases minus what the read-backs of the device's
        // cursor have shown to be unused), the worst cases added up, and the device's cursor itself (synchronises the compute stream)
        DeviceGuard g(e->device);
        if (!strcmp(name, "arena_cursor")) {
            uint32_t c = 0;
            HIP_TRY(hipStreamSynchronize(e->s_compute));
            if (e->tp.d_cursor && e->tp.pending) HIP_TRY(hipMemcpy(&c, e->tp.d_cursor, sizeof c, hipMemcpyDeviceToHost));
            *value = (int64_t)c; return KDB_OK;
        }
        kdb::twolevel_paged_poll(e->tp);
        *value = (int64_t)(!strcmp(name, "arena_worst_case") ? e->tp.used2 : e->tp.used2 - e->tp.slack); return KDB_OK;
    }
    {
        // HBM traffic by the engine's own account (cumulative since kdb_reset; the device is synchronised to read them)
        static const struct { const char *name; size_t off; } dev[] = {
            {"pages_bases", offsetof(kdb::DevCounters, pages_bases)}, {"lines_bases", offsetof(kdb::DevCounters, lines_bases)},
            {"pages_ids", offsetof(kdb::DevCounters, pages_ids)},     {"lines_ids", offsetof(kdb::DevCounters, lines_ids)},
            {"table_bytes", offsetof(kdb::DevCounters, table_bytes)}, {"total_kmers", offsetof(kdb::DevCounters, total_kmers)}};
        for (const auto &d : dev)
            if (!strcmp(name, d.name)) {
                DeviceGuard g(e->device);
                HIP_TRY(hipStreamSynchronize(e->s_compute));
                unsigned long long v = 0;
                HIP_TRY(hipMemcpy(&v, (const char *)e->d_ctr + d.off, sizeof v, hipMemcpyDeviceToHost));
                *value = (int64_t)v;
                return KDB_OK;
            }
    }
    return fail(KDB_ERR_ARG, "unknown option '%s'", name);
}

}  // extern "C"
