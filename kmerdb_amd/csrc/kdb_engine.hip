// kdb_engine.hip -- the one translation unit of libkdbhip.so and the host side of its engine: the engine object (HBM count vector,
// streams, pinned double-buffered staging), the launches of a batch, the submits, sync and reset, the readers, reduce and fold, and the
// ids calls.  The other jobs of include/kdbhip.h are headers included here: kdb_io_abi.hip.h (parsers, gzip, .kdb files),
// kdb_probe_host.hip.h (the HBM pattern probe), kdb_engine_options.hip.h (the option table) and kdb_analysis_host.hip.h (the analysis
// calls).  gfx950 only; no CPU fallback: every entry point that needs the device fails with KDB_ERR_HIP if HIP cannot provide one.
#include <hip/hip_runtime.h>

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
#include "kdb_hostutil.hip.h"
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
#include "kdb_strands.hip.h"
#include "kdb_score.hip.h"
#include "kdb_tables.hip.h"
#include "kdb_minimizers.hip.h"
#include "kdb_align.hip.h"
#include "kdb_hostparse.cpp.h"
#include "kdb_kdbwriter.cpp.h"
#include "kdb_submit_plan.cpp.h"
#include "kdb_io_abi.hip.h"
#include "kdb_probe_host.hip.h"

namespace {

constexpr int NBUF = 2;                                  // double-buffered staging
const char *const KERNEL_NAMES[KDB_N_KERNELS] = {
    "lens+mark_reads_kernel", "count_kernel", "scatter_bases_kernel", "scatter_ids_kernel", "pages_sort_kernels", "page_hist_kernel", "stats_kernel", "strand_merge_kernel"};
const char *const NO_VECTOR = "created by kdb_create_ids: it has no count vector";

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

// ---- how host memory reaches the device: the staging pair, the accumulated batch behind it, and the ring of a pinned caller ----
struct StageSlot {
    PinnedBuf<uint8_t> h_bases; PinnedBuf<uint64_t> h_offs;
    DevBuf<uint8_t> d_bases; DevBuf<uint64_t> d_offs;
    Event ev_copied, ev_done;
    hipEvent_t busy = nullptr;       // what must complete before the slot is reused: ev_copied (appended to the accumulated batch) or ev_done (counted from here)
    bool inflight = false;
};

// device-side accumulation of staged chunks (large k: every batch pays one sweep of the 4^k vector in P2,
// so 64 MiB batches would be dominated by it; chunks are appended here and counted as one batch)
struct AccSlot { DevBuf<uint8_t> bases; DevBuf<uint64_t> offs; Event ev_done; bool inflight = false; };

// kdb_submit_pinned: the DMA reads the caller's buffer; call N waits for the copies of call N-2, so a caller that
// cycles through three buffers (kmerdb_amd.reader) can never overwrite one that is still being read
struct PinRing { Event ev[2]; bool used[2] = {false, false}; int idx = 0; };

struct HostFeed {
    size_t stage_bytes = 64ull << 20, stage_reads = 2ull << 20;
    int64_t accum_bytes = -1;                        // -1 auto (1 GiB for k >= 13, off below), 0 off
    StageSlot stage[NBUF];
    int next_buf = 0;
    bool staging_ready = false;                      // allocated on the first kdb_submit
    size_t acc_cap = 0, acc_reads_cap = 0;
    AccSlot acc[2];
    Event ev_acc_copied;
    int acc_slot = 0;
    size_t acc_nb = 0, acc_nr = 0;
    bool acc_ready = false;
    PinRing pin;

    int ensure_staging(int k)
    {
        if (staging_ready) return KDB_OK;
        for (StageSlot &s : stage) {
            HIP_TRY(s.h_bases.alloc(stage_bytes + 64));
            HIP_TRY(s.h_offs.alloc((stage_reads + 1) * sizeof(uint64_t)));
            HIP_TRY(s.d_bases.alloc(stage_bytes + 64));
            HIP_TRY(s.d_offs.alloc((stage_reads + 1) * sizeof(uint64_t)));
            HIP_TRY(s.ev_copied.create());
            HIP_TRY(s.ev_done.create());
        }
        staging_ready = true;
        // (from k = 13 on every batch pays a sweep of the 4^k vector -- 0.5 GiB at k = 13 -- or, on the two-level path, partial pages of
        //  512 rings x 512 workgroups: 64 MiB chunks are appended on the device and counted 1 GiB at a time)
        const int64_t want = accum_bytes >= 0 ? accum_bytes : (k >= 13 ? (int64_t)1 << 30 : 0);
        if (want > 0) {
            acc_cap = (size_t)want < stage_bytes ? stage_bytes : (size_t)want;
            acc_reads_cap = acc_cap / 64 + stage_reads;
            for (AccSlot &a : acc) {
                HIP_TRY(a.bases.alloc(acc_cap + 64));
                HIP_TRY(a.offs.alloc((acc_reads_cap + 1) * sizeof(uint64_t)));
                HIP_TRY(a.ev_done.create());
            }
            HIP_TRY(ev_acc_copied.create());
            acc_ready = true;
        }
        return KDB_OK;
    }

    // a piece of whole records goes behind the accumulated batch if it could ever fit one
    bool appends(const kdbplan::SubmitPiece &p) const
    {
        return acc_ready && !p.first_is_continuation && !p.ends_inside_record && p.nbytes <= acc_cap && p.nrecs <= acc_reads_cap;
    }

    void idle()                                      // the streams have been synchronised: nothing is in flight
    {
        for (StageSlot &s : stage) s.inflight = false;
        for (AccSlot &a : acc) a.inflight = false;
    }
};

}  // namespace

// Members are destroyed last to first: the two streams stand first so that they go last, behind everything that was used on them.
struct kdb_engine {
    Stream s_copy, s_compute;
    int k = 0, canonical = 1, n_mode = KDB_N_DROP, device = 0;
    uint64_t nbins = 0;
    unsigned long long *d_table = nullptr;           // the caller's vector, or own_table's
    DevBuf<unsigned long long> own_table;
    bool owns_table = false;
    bool table_escaped = false;      // kdb_table handed the vector's address out: the caller may write it at any time
    DevBuf<kdb::DevCounters> d_ctr;
    bool batch_words_zero = false;                                    // the per-batch words of d_ctr are zero: kdb_reset, or the batch before ended in resolve_suspects_kernel
    DevBuf<unsigned long long> d_worklist;           // EXPAND mode: windows with > 2 N's, expanded by a workgroup each
    size_t worklist_cap = 1u << 20;
    DevBuf<uint32_t> d_first_rec;                    // record that holds every 4096th byte of the batch in hand (lens_kernel)
    DevBuf<unsigned long long> d_suspects;           // DROP mode: positions of a batch's residues that are neither ACGT nor N (resolve_suspects_kernel)
    DevBuf<unsigned long long> sh_suspects;          // the same for kdb_shred / kdb_window_ids
    size_t suspects_cap = 1u << 16;

    HostFeed feed;
    int copy_threads = 8;

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
    Stream s_hist;
    kdb::OverlapState ov;
    kdb::TwoLevelPaged tp;            // its two-level form (k = 13..17): level-1 scratch and the arena of pending level-2 pages
    kdb::OneLevelPending ol;          // the one-level path with option one_level_defer: the arena of batches scattered but not yet added to the vector
    int64_t oom_fallbacks = 0;        // batches that fell back to direct atomics because scratch did not fit
    // canonical engines, one-level LDS-histogram paths: batches count forward ids into d_fwd, kdb_sync adds both strands to d_table
    // at the canonical bins (kdb_strands.hip.h).  d_table itself is only ever added to, at canonical bins, as without the staging.
    int strand_merge = 1;             // 0: min(fwd, rc) per window in the counting kernels, straight into d_table
    int strand_merge_max_k = 12;      // the largest k that is staged (never more than one_level_max_k); k = 13 measured no faster, DESIGN.md section 4
    DevBuf<unsigned long long> d_fwd;                // 4^k uint64, allocated at the first staged batch; all zero unless strands_pending
    bool strands_pending = false;

    // ids-only engines (kdb_create_ids) have no count vector; scratch of kdb_shred / kdb_window_ids (grow-only)
    bool tableless = false;
    DevBuf<uint8_t> sh_seq;
    DevBuf<uint64_t> sh_offs;
    DevBuf<unsigned long long> sh_ids;
    DevBuf<kdb::DevCounters> sh_ctr;

    // samplesheet accumulator (kdb_fold_file): counts = counts + counts_ stays on the device
    DevBuf<unsigned long long> d_acc_table;
    uint64_t folded_files = 0, folded_total = 0;
    uint64_t d2h_bytes = 0;           // bytes of count vector copied to the host so far (tests assert "one copy at the end")
    uint64_t bytes_in = 0;            // residue bytes handed to the counting kernels so far

    // profiling
    bool prof = false;
    std::vector<ProfSpan> spans;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[KDB_N_KERNELS] = {0};
    uint64_t prof_n[KDB_N_KERNELS] = {0};

    // with the engine's device selected (kdb_destroy): the streams run dry, the histogram stream and the scatter paths' state go, then
    // the members, the two streams last
    ~kdb_engine()
    {
        if (s_compute) (void)hipStreamSynchronize(s_compute);
        if (s_copy) (void)hipStreamSynchronize(s_copy);
        if (s_hist) { (void)hipStreamSynchronize(s_hist); (void)s_hist.destroy(); }
        kdb::overlap_free(ov);
        kdb::scatter_free(sc);
        kdb::twolevel_paged_free(tp);
        kdb::one_level_free(ol);
        for (auto &s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
        for (auto ev : ev_pool) (void)hipEventDestroy(ev);
    }
};

namespace {

hipEvent_t prof_event(kdb_engine *e)
{
    hipEvent_t ev = nullptr;
    if (!e->ev_pool.empty()) { ev = e->ev_pool.back(); e->ev_pool.pop_back(); return ev; }
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return ev;
}

struct ProfScope {
    kdb_engine *e; int kernel; hipStream_t stream; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(kdb_engine *e_, int kernel_, hipStream_t stream_ = nullptr) : e(e_), kernel(kernel_), stream(stream_ ? stream_ : e_->s_compute.s)
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

int no_vector() { return fail(KDB_ERR_STATE, "this engine was %s", NO_VECTOR); }

// How an entry point that takes an engine begins: NULL, no count vector where the call reads or writes one, the call's own refusals,
// then -- on the engine's device -- kdb_sync where the call begins with one, and the call itself.
enum : int { NEEDS_VECTOR = 1, SYNCS_FIRST = 2 };
template <class Refusals, class Body>
int engine_call(kdb_engine *e, int flags, Refusals refusals, Body body)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if ((flags & NEEDS_VECTOR) && e->tableless) return no_vector();
    if (const int rc = refusals()) return rc;
    DeviceGuard g(e->device);
    if (flags & SYNCS_FIRST) { const int rc = kdb_sync(e); if (rc != KDB_OK) return rc; }
    return body();
}
template <class Body>
int engine_call(kdb_engine *e, int flags, Body body) { return engine_call(e, flags, [] { return KDB_OK; }, body); }

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
    if (e->s_hist) { HIP_TRY(hipStreamSynchronize(e->s_hist)); HIP_TRY(e->s_hist.destroy()); }
    kdb::overlap_free(e->ov);
    if (e->compute_masked || want_mask) {
        HIP_TRY(hipStreamSynchronize(e->s_compute));
        HIP_TRY(e->s_compute.destroy());
        e->compute_masked = false;
    }
    if (!want_hist) {
        if (!e->s_compute) HIP_TRY(e->s_compute.create());
        return KDB_OK;
    }
    if (!want_mask) {
        if (!e->s_compute) HIP_TRY(e->s_compute.create());
        HIP_TRY(e->s_hist.create());
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
    HIP_TRY(hipExtStreamCreateWithCUMask(&e->s_compute.s, (uint32_t)ms.size(), ms.data()));
    e->compute_masked = true;
    HIP_TRY(hipExtStreamCreateWithCUMask(&e->s_hist.s, (uint32_t)mh.size(), mh.data()));
    e->ov.grid = 2u * (uint32_t)(ncu - given);                 // two persistent scatter workgroups per CU of the compute stream
    return KDB_OK;
}

// the staging vector of forward counts, allocated and zeroed at its first use.  No room for it: the batch in hand is counted canonically
// into d_table as without it (not an oom_fallback: no scratch was refused), and the next batch asks again.
bool ensure_fwd(kdb_engine *e)
{
    if (e->d_fwd) return true;
    if (e->d_fwd.alloc(e->nbins * 8ull) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipMemsetAsync(e->d_fwd, 0, e->nbins * 8ull, e->s_compute) != hipSuccess) { (void)hipGetLastError(); e->d_fwd.release(); return false; }
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

// ---- one device-resident batch through the counting kernels, on s_compute: launch_batch and its steps, in the order they run ----
enum : int { BATCH_HOST_FED = 1, BATCH_CONST_INPUT = 2 };
struct Batch {
    uint8_t *d_bases; size_t nbytes; const uint64_t *d_offs; size_t nreads; int first_is_continuation, flags;
    // The LDS-histogram paths take a ragged batch's record starts from the offsets (lens_kernel fills first_rec; nothing is written
    // into the residues).  Only the direct-atomics kernel (algo 1, or the fallback when the scatter scratch does not fit) and the
    // old k <= 7 kernel still mark record starts as bit 7 of a record's first byte: the marks go on right before such a kernel and
    // come off again right after it.
    bool marked = false;
};

void mark(kdb_engine *e, Batch &b)
{
    ProfScope ps(e, KDB_KERNEL_MARK);
    const unsigned mg = (unsigned)std::min<uint64_t>((b.nreads + 255) / 256, 4096);
    if (b.flags & BATCH_CONST_INPUT)          // the caller's buffer is never written: these kernels then need records of one length
        hipLaunchKernelGGL(kdb::require_uniform_kernel, dim3(1), dim3(1), 0, e->s_compute, e->d_ctr.p);
    else {
        hipLaunchKernelGGL(kdb::mark_reads_kernel, dim3(mg), dim3(256), 0, e->s_compute, b.d_bases, b.d_offs, (uint64_t)b.nreads,
                           b.first_is_continuation, e->d_ctr.p);          // (grid-stride: a uniform batch returns at once)
        b.marked = true;
    }
}

void unmark(kdb_engine *e, Batch &b)
{
    if (!b.marked) return;
    ProfScope ps(e, KDB_KERNEL_MARK);
    const unsigned ug = (unsigned)std::min<uint64_t>((b.nreads + 255) / 256, 4096);
    hipLaunchKernelGGL(kdb::unmark_reads_kernel, dim3(ug), dim3(256), 0, e->s_compute, b.d_bases, b.d_offs, (uint64_t)b.nreads, b.first_is_continuation,
                       (const kdb::DevCounters *)e->d_ctr.p);
    b.marked = false;
}

// first_rec: one entry per 4 KiB of residues (grow-only scratch).  The batch before this one may still be reading the old array
// (submits of device-resident input are asynchronous): drain the stream before it is freed.  No room for a larger one (*none): the
// direct-atomics kernel needs none, the batch is counted there (as when the scatter scratch does not fit).
int first_rec_scratch(kdb_engine *e, size_t nbytes, bool *none)
{
    const size_t need = ((nbytes >> kdb::FIRST_REC_SHIFT) + 2) * sizeof(uint32_t);
    if (e->d_first_rec.cap < need && e->d_first_rec) HIP_TRY(hipStreamSynchronize(e->s_compute));
    const int rc = e->d_first_rec.grow(need);
    *none = rc == KDB_ERR_NOMEM;
    return *none ? KDB_OK : rc;
}

// the batch's own counter words, then record lengths, layout and first_rec
int lens_and_batch_words(kdb_engine *e, const Batch &b)
{
    ProfScope ps(e, KDB_KERNEL_MARK);
    const dim3 grid((unsigned)((b.nreads + 255) / 256)), block(256);
    // only the per-batch words: n_short, n_bad, bad_layout, not_uniform stay set until kdb_reset.  (Where the batch before ended in
    // resolve_suspects_kernel, that kernel has left them zero: no memset, one dispatch less per batch.)
    if (!e->batch_words_zero) HIP_TRY(hipMemsetAsync(&e->d_ctr->neg_min_len, 0, kdb::PER_BATCH_WORDS * sizeof(unsigned long long), e->s_compute));
    e->batch_words_zero = false;
    const dim3 lgrid(grid.x < 1024u ? grid.x : 1024u);
    hipLaunchKernelGGL(kdb::lens_kernel, lgrid, block, 0, e->s_compute, b.d_offs, (uint64_t)b.nreads, (uint64_t)b.nbytes,
                       e->min_len > 0 ? e->min_len : e->k, b.first_is_continuation, e->d_ctr.p, e->d_first_rec.p);
    // bytes with bit 7 set are no residues (kmer.py:170 raises).  No pass of its own looks for them: the counting kernels'
    // front end counts them as bad; where the direct-atomics kernel runs over a ragged batch (its start marks are bit 7),
    // mark_reads_kernel reports a record start that carries the bit already, and any other such byte is a mark too many
    // (marks_seen != marks_set at the sync).  Host-fed and device-resident input alike.
    return KDB_OK;
}

// The LDS-histogram path of the engine's k and options.  0: counted (or scattered, to be counted later); 2: no room for its scratch,
// the batch goes to the direct kernel; else an error of the path or a status of overlap_join.
int route_lds(kdb_engine *e, Batch &b, const kdb::RecStarts &rs, int canonical, unsigned long long *table, int *status)
{
    EngineProf hook(e);
    const bool ex = e->n_mode == KDB_N_EXPAND;
    const kdb::ScBatch batch{b.d_bases, b.nbytes, rs, e->k, canonical, ex, table, e->d_ctr};
    int rc;
    if (e->k <= kdb::SMALLK_LDS_MAX_K && !e->smallk_old)
        rc = kdb::smallk_lds_count(e->s_compute, b.d_bases, b.nbytes, rs, e->k, canonical, ex, e->opt.grid, table, e->d_ctr, hook);
    else if (e->k <= kdb::SMALLK_MAX) {
        mark(e, b);
        rc = kdb::smallk_count(e->s_compute, b.d_bases, b.nbytes, e->k, canonical, ex, table, e->d_ctr, hook);
        unmark(e, b);
    }
    else if (e->k <= e->opt.one_level_max_k) {
        rc = 3;
        if (e->overlap && e->s_hist && !ex) rc = kdb::scatter_count_overlapped(e->ov, e->opt, e->s_compute, e->s_hist, batch, hook);
        if (rc == 3) {
            if ((*status = overlap_join(e)) != KDB_OK) return 1;
            // (one_level_defer: stage 2 waits for more batches; 3 = no room for an arena of two regions, and nothing is pending)
            if (kdb::one_level_depth(e->opt, e->k) >= 2 && !(e->overlap && e->s_hist)) rc = kdb::scatter_count_deferred(e->ol, e->opt, e->s_compute, batch, hook);
            if (rc == 3) rc = kdb::scatter_count(e->sc, e->opt, e->s_compute, batch, hook);
        }
    }
    else {
        const size_t lost = b.nreads * (size_t)(e->k - 1);
        rc = kdb::twolevel_paged_count(e->tp, e->opt, e->s_compute, batch, b.nbytes > lost ? b.nbytes - lost : 0, hook);
    }
    if (rc != 0 && rc != 2) *status = fail(KDB_ERR_HIP, "LDS-histogram path failed: %s", kdb::partition_error());
    return rc;
}

void count_direct(kdb_engine *e, Batch &b, uint64_t ntiles, int canonical, unsigned long long *table)
{
    mark(e, b);
    {
        ProfScope ps(e, KDB_KERNEL_COUNT);
        const bool ex = (e->n_mode == KDB_N_EXPAND);
        const dim3 grid((unsigned)ntiles), block(kdb::TPB);
#define KDB_LAUNCH_DIRECT(ID, EX)                                                                              \
    hipLaunchKernelGGL((kdb::count_direct_kernel<ID, EX>), grid, block, 0, e->s_compute, b.d_bases, (uint64_t)b.nbytes, \
                       e->k, canonical, table, e->d_ctr.p)
        if (e->k <= 16) { if (ex) KDB_LAUNCH_DIRECT(uint32_t, true); else KDB_LAUNCH_DIRECT(uint32_t, false); }
        else            { if (ex) KDB_LAUNCH_DIRECT(uint64_t, true); else KDB_LAUNCH_DIRECT(uint64_t, false); }
#undef KDB_LAUNCH_DIRECT
    }
    unmark(e, b);
}

// what the counting kernels left for later: EXPAND mode's worklist, DROP mode's suspects
int batch_tail(kdb_engine *e, const Batch &b, int canonical, unsigned long long *table)
{
    if (e->n_mode == KDB_N_EXPAND && e->d_worklist) {
        ProfScope ps(e, KDB_KERNEL_COUNT);
        hipLaunchKernelGGL(kdb::expand_worklist_kernel, dim3(1024), dim3(256), 0, e->s_compute, table, e->d_ctr.p, e->k, canonical);
    }
    if (e->n_mode == KDB_N_DROP) {
        // residues that are neither ACGT nor N: an IUPAC code is only an error in a window that no N shields (kmer.py:287-289)
        ProfScope ps(e, KDB_KERNEL_MARK);
        hipLaunchKernelGGL(kdb::resolve_suspects_kernel, dim3(4), dim3(256), 0, e->s_compute, (const uint8_t *)b.d_bases, (uint64_t)b.nbytes, b.d_offs, (uint64_t)b.nreads,
                           e->k, e->d_ctr.p, 1);
        HIP_TRY(hipGetLastError());
        e->batch_words_zero = true;              // (the batch's last kernel: it puts the per-batch words back to zero)
        return KDB_OK;
    }
    HIP_TRY(hipGetLastError());
    return KDB_OK;
}

int launch_batch(kdb_engine *e, uint8_t *d_bases, size_t nbytes, const uint64_t *d_offs, size_t nreads, int first_is_continuation, int flags)
{
    if (nreads == 0) return KDB_OK;
    if (e->tableless) return no_vector();
    const uint64_t ntiles = (nbytes + kdb::TILE_BYTES - 1) / kdb::TILE_BYTES;
    if (ntiles > 0x7FFFFFFFull) return fail(KDB_ERR_ARG, "batch too large: %zu bytes", nbytes);       // (before anything is written into the caller's buffer)
    Batch b{d_bases, nbytes, d_offs, nreads, first_is_continuation, flags};
    bool no_first_rec = false;
    int rc;
    if ((rc = first_rec_scratch(e, nbytes, &no_first_rec)) != KDB_OK) return rc;
    if ((rc = lens_and_batch_words(e, b)) != KDB_OK) return rc;
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
    unsigned long long *const table = staged ? e->d_fwd.p : e->d_table;
    if (staged) e->strands_pending = true;
    if (algo == 2) {
        int status = KDB_OK;
        const int lrc = route_lds(e, b, rs, canonical, table, &status);
        if (lrc == 2) { e->oom_fallbacks++; algo = 1; e->tp.table_is_zero = false; }   // no room for the scatter scratch: count this batch with direct atomics
        else if (lrc != 0) return status;
    }
    if (algo == 1) {
        if ((rc = overlap_join(e)) != KDB_OK) return rc;
        count_direct(e, b, ntiles, canonical, table);
    }
    return batch_tail(e, b, canonical, table);
}

// count what has been accumulated so far as one batch
int flush_accumulated(kdb_engine *e)
{
    HostFeed &f = e->feed;
    if (!f.acc_ready || f.acc_nr == 0) return KDB_OK;
    AccSlot &a = f.acc[f.acc_slot];
    HIP_TRY(hipEventRecord(f.ev_acc_copied, e->s_copy));
    HIP_TRY(hipStreamWaitEvent(e->s_compute, f.ev_acc_copied, 0));
    int rc = launch_batch(e, a.bases, f.acc_nb, a.offs, f.acc_nr, 0, BATCH_HOST_FED);
    if (rc != KDB_OK) return rc;
    HIP_TRY(hipEventRecord(a.ev_done, e->s_compute));
    a.inflight = true;
    f.acc_slot ^= 1;
    f.acc_nb = f.acc_nr = 0;
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

void stats_sweep(kdb_engine *e, const unsigned long long *vec)
{
    unsigned grid = (unsigned)((e->nbins + 255) / 256);
    if (grid > 256u * 16u) grid = 256u * 16u;
    hipLaunchKernelGGL(kdb::stats_kernel, dim3(grid), dim3(256), 0, e->s_compute, vec, e->nbins, e->d_ctr.p);
}

// The tail of every reader of a vector: `sweep` (stats_kernel over `vec`, or the fold) adds count_nonzero and Sum to the zeroed
// counters, the vector is optionally copied to the host, the results are left in *c.  emitted: Sum must equal the k-mers emitted.
template <class Sweep>
int vector_stats(kdb_engine *e, const unsigned long long *vec, uint64_t *counts_out, kdb::DevCounters *c, bool emitted, Sweep sweep)
{
    HIP_TRY(hipMemsetAsync(&e->d_ctr->unique, 0, 2 * sizeof(unsigned long long), e->s_compute));
    {
        ProfScope ps(e, KDB_KERNEL_STATS);
        sweep();
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
    if (emitted && c->sum != c->total_kmers)
        return fail(KDB_ERR_STATE, "internal: Sum(counts)=%llu but %llu k-mers were emitted", c->sum, c->total_kmers);
    return KDB_OK;
}

int nullomers(kdb_engine *e, const unsigned long long *vec, uint64_t *ids_out, uint64_t cap, uint64_t *n_out)
{
    if (((uintptr_t)vec & 15u) != 0) return fail(KDB_ERR_ARG, "the count vector must be 16-byte aligned for kdb_nullomers");
    const uint64_t ntiles = (e->nbins + kdb::NULL_TILE - 1) / kdb::NULL_TILE;
    const uint64_t nranges = (ntiles + kdb::NULL_RANGE_TILES - 1) / kdb::NULL_RANGE_TILES;
    struct Scratch { DevBuf<uint32_t> tile_counts; DevBuf<unsigned long long> range_totals, out[2]; Event written[2], copied[2]; } sc;
    if (sc.tile_counts.alloc(ntiles * sizeof(uint32_t)) != hipSuccess || sc.range_totals.alloc(nranges * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KDB_ERR_NOMEM, "kdb_nullomers: no room for %llu tile counts", (unsigned long long)ntiles);
    }
    hipLaunchKernelGGL(kdb::null_count_kernel, dim3((unsigned)std::min<uint64_t>(ntiles, 256u * 16u)), dim3(kdb::NULL_TPB), 0, e->s_compute, vec, e->nbins, ntiles, sc.tile_counts.p);
    hipLaunchKernelGGL(kdb::null_scan_kernel, dim3((unsigned)nranges), dim3(1024), 0, e->s_compute, sc.tile_counts.p, ntiles, sc.range_totals.p);
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
        if (sc.out[b].alloc(largest * 8ull) != hipSuccess) { (void)hipGetLastError(); return fail(KDB_ERR_NOMEM, "kdb_nullomers: no room for %llu ids on the device", (unsigned long long)largest); }
        HIP_TRY(sc.written[b].create());
        HIP_TRY(sc.copied[b].create());
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
                           (const uint32_t *)sc.tile_counts.p, sc.out[b].p);
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

// kdb_shred (offs NULL: the residues are one record) and kdb_window_ids: the residues and offsets go up, the counter block is cleared
// and given its suspects list, the kernels run -- what looks at records only with offsets, the grids each call's own --, the ids of all
// nbytes positions come down into ids_out, and what the kernels counted is refused.
int window_ids_run(kdb_engine *e, const uint8_t *seq, size_t nbytes, const uint64_t *offs, size_t nreads, unsigned long long *ids_out)
{
    int rc;
    if ((rc = e->sh_seq.grow(nbytes + 64)) != KDB_OK) return rc;
    if ((rc = e->sh_ids.grow(nbytes * 8ull)) != KDB_OK) return rc;
    if (offs && (rc = e->sh_offs.grow((nreads + 1) * sizeof(uint64_t))) != KDB_OK) return rc;
    if (!e->sh_ctr) HIP_TRY(e->sh_ctr.alloc(sizeof(kdb::DevCounters)));
    if (!e->sh_suspects) HIP_TRY(e->sh_suspects.alloc(e->suspects_cap * sizeof(unsigned long long)));
    kdb::DevCounters c;
    memset(&c, 0, sizeof c);
    const unsigned long long sus[2] = {(unsigned long long)(uintptr_t)e->sh_suspects.p, (unsigned long long)e->suspects_cap};
    HIP_TRY(hipMemcpyAsync(e->sh_seq, seq, nbytes, hipMemcpyHostToDevice, e->s_compute));
    if (offs) HIP_TRY(hipMemcpyAsync(e->sh_offs, offs, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->s_compute));
    HIP_TRY(hipMemsetAsync(e->sh_ctr, 0, sizeof c, e->s_compute));
    HIP_TRY(hipMemcpyAsync(&e->sh_ctr->sus, sus, sizeof sus, hipMemcpyHostToDevice, e->s_compute));
    const dim3 grid((unsigned)((nreads + 255) / 256)), block(256), lgrid(grid.x < 1024u ? grid.x : 1024u);
    if (offs)
        hipLaunchKernelGGL(kdb::lens_kernel, lgrid, block, 0, e->s_compute, e->sh_offs.p, (uint64_t)nreads, (uint64_t)nbytes,
                           e->min_len > 0 ? e->min_len : e->k, 0, e->sh_ctr.p, (uint32_t *)nullptr);
    hipLaunchKernelGGL(kdb::hibit_check_kernel, dim3(offs ? 1024 : 64), dim3(256), 0, e->s_compute, e->sh_seq.p, (uint64_t)nbytes, e->sh_ctr.p);
    if (offs)
        hipLaunchKernelGGL(kdb::mark_reads_kernel, dim3(grid.x < 4096u ? grid.x : 4096u), block, 0, e->s_compute, e->sh_seq.p, e->sh_offs.p, (uint64_t)nreads, 0,
                           e->sh_ctr.p);
    const unsigned ntiles = (unsigned)((nbytes + kdb::TILE_BYTES - 1) / kdb::TILE_BYTES);
    hipLaunchKernelGGL(kdb::shred_kernel, dim3(ntiles), dim3(kdb::TPB), 0, e->s_compute, e->sh_seq.p, (uint64_t)nbytes, e->k,
                       e->canonical, e->sh_ids.p, e->sh_ctr.p);
    hipLaunchKernelGGL(kdb::resolve_suspects_kernel, dim3(offs ? 4 : 1), dim3(256), 0, e->s_compute, (const uint8_t *)e->sh_seq.p, (uint64_t)nbytes,
                       (const uint64_t *)(offs ? e->sh_offs.p : nullptr), (uint64_t)nreads, e->k, e->sh_ctr.p, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ids_out, e->sh_ids, nbytes * 8ull, hipMemcpyDeviceToHost, e->s_compute));
    HIP_TRY(hipMemcpyAsync(&c, e->sh_ctr, sizeof c, hipMemcpyDeviceToHost, e->s_compute));
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    if (offs && c.bad_layout) return fail(KDB_ERR_ARG, "read_offsets must rise from 0 to nbytes");
    if (offs && c.n_short) return fail(KDB_ERR_SHORT_READ, "%llu record(s) shorter than k=%d (reference: kmer.py:461-463 raises)", c.n_short, e->k);
    if (c.n_bad) return fail(KDB_ERR_BAD_RESIDUE, "%llu residue(s) outside ACGTN (reference: kmer.py:309 / :170 raises)", c.n_bad);
    return KDB_OK;
}

int engine_env_options(kdb_engine *e);

int create_common(kdb_engine *e, kdb_engine **out)
{
    hipError_t err;
    if ((err = e->s_compute.create()) != hipSuccess || (err = e->s_copy.create()) != hipSuccess ||
        (err = e->d_ctr.alloc(sizeof(kdb::DevCounters))) != hipSuccess) {
        kdb_destroy(e);
        return fail(KDB_ERR_HIP, "engine setup failed: %s", hipGetErrorString(err));
    }
    int rc = kdb_reset(e);
    if (rc == KDB_OK) rc = engine_env_options(e);
    if (rc != KDB_OK) { kdb_destroy(e); return rc; }
    *out = e;
    return KDB_OK;
}

}  // namespace

#include "kdb_engine_options.hip.h"

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

// what both kinds of engine are created from, once the arguments pass (why_k: the end of the message that refuses k)
static int new_engine(int k, const char *why_k, int canonicalize, int n_mode, int device_id, kdb_engine **out, kdb_engine **e_out)
{
    if (!out) return fail(KDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (k < 1 || k > 17) return fail(KDB_ERR_ARG, "k=%d outside 1..17%s", k, why_k);
    if (n_mode != KDB_N_DROP && n_mode != KDB_N_EXPAND) return fail(KDB_ERR_ARG, "n_mode=%d", n_mode);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    kdb_engine *e = *e_out = new kdb_engine();
    e->k = k; e->canonical = canonicalize ? 1 : 0; e->n_mode = n_mode; e->device = device_id;
    return KDB_OK;
}

int kdb_create(int k, int canonicalize, int n_mode, int device_id, void *d_table, kdb_engine **out)
{
    // (the histogram pass of the paged paths moves the vector in 16-byte pieces, hist_flush_runs; which path counts a batch is decided later)
    if (out && ((uintptr_t)d_table & 15u) != 0) { *out = nullptr; return fail(KDB_ERR_ARG, "d_table must be 16-byte aligned"); }
    kdb_engine *e = nullptr;
    const int rc = new_engine(k, " (4^k uint64 table must fit in HBM)", canonicalize, n_mode, device_id, out, &e);
    if (rc != KDB_OK) return rc;
    DeviceGuard g(device_id);
    e->nbins = 1ull << (2 * k);
    if (d_table) {
        e->d_table = (unsigned long long *)d_table;
        e->owns_table = false;
    } else {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        const unsigned long long need = e->nbins * 8ull;
        if (free_b && need > free_b) {
            kdb_destroy(e);
            return fail(KDB_ERR_NOMEM, "4^%d uint64 table needs %llu bytes, device has %zu free", k, need, free_b);
        }
        hipError_t me = e->own_table.alloc(need);
        if (me != hipSuccess) { kdb_destroy(e); return fail(KDB_ERR_NOMEM, "hipMalloc(%llu) failed: %s", need, hipGetErrorString(me)); }
        e->d_table = e->own_table;
        e->owns_table = true;
    }
    return create_common(e, out);
}

int kdb_create_ids(int k, int canonicalize, int device_id, kdb_engine **out)
{
    kdb_engine *e = nullptr;
    const int rc = new_engine(k, "", canonicalize, KDB_N_DROP, device_id, out, &e);
    if (rc != KDB_OK) return rc;
    DeviceGuard g(device_id);
    e->nbins = 0; e->tableless = true;
    return create_common(e, out);
}

int kdb_destroy(kdb_engine *e)
{
    if (!e) return KDB_OK;
    DeviceGuard g(e->device);
    delete e;                                        // (~kdb_engine: the order in which things go)
    return KDB_OK;
}

int kdb_reset(kdb_engine *e)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    DeviceGuard g(e->device);
    e->feed.acc_nb = e->feed.acc_nr = 0;             // anything not yet counted is dropped with the vector
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
    e->batch_words_zero = true;
    unsigned long long wl[2] = {0, 0}, sus[2] = {0, 0};
    if (e->n_mode == KDB_N_EXPAND) {
        if (!e->d_worklist) HIP_TRY(e->d_worklist.alloc(e->worklist_cap * sizeof(unsigned long long)));
        wl[0] = (unsigned long long)(uintptr_t)e->d_worklist.p; wl[1] = (unsigned long long)e->worklist_cap;
        HIP_TRY(hipMemcpyAsync(&e->d_ctr->wl, wl, sizeof wl, hipMemcpyHostToDevice, e->s_compute));
    } else if (!e->tableless) {
        if (!e->d_suspects) HIP_TRY(e->d_suspects.alloc(e->suspects_cap * sizeof(unsigned long long)));
        sus[0] = (unsigned long long)(uintptr_t)e->d_suspects.p; sus[1] = (unsigned long long)e->suspects_cap;
        HIP_TRY(hipMemcpyAsync(&e->d_ctr->sus, sus, sizeof sus, hipMemcpyHostToDevice, e->s_compute));
    }
    HIP_TRY(hipStreamSynchronize(e->s_compute));
    return KDB_OK;
}

static int submit_device(kdb_engine *e, const void *d_bases, size_t nbytes, const void *d_read_offsets, size_t nreads, int flags)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (nreads && (!d_bases || !d_read_offsets)) return fail(KDB_ERR_ARG, "NULL device buffer");
    if (((uintptr_t)d_bases & 15u) != 0) return fail(KDB_ERR_ARG, "d_bases must be 16-byte aligned");
    DeviceGuard g(e->device);
    return launch_batch(e, (uint8_t *)const_cast<void *>(d_bases), nbytes, (const uint64_t *)d_read_offsets, nreads, 0, flags);
}

int kdb_submit_device(kdb_engine *e, void *d_bases, size_t nbytes, const void *offs, size_t nreads) { return submit_device(e, d_bases, nbytes, offs, nreads, 0); }

// (the caller's buffer is never written)
int kdb_submit_device_const(kdb_engine *e, const void *d_bases, size_t nbytes, const void *offs, size_t nreads) { return submit_device(e, d_bases, nbytes, offs, nreads, BATCH_CONST_INPUT); }

// One host-fed submit: the cut into pieces is kdbplan::SubmitCutter's; per piece, wait for the staging slot, let the cutter write the
// piece's offsets into it, copy, and either append the piece to the accumulated batch or count it from the slot.
static int submit_impl(kdb_engine *e, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads, bool src_pinned, bool first_continues = false)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    if (nreads == 0) return KDB_OK;
    if (!offs || (!bases && nbytes)) return fail(KDB_ERR_ARG, "NULL host buffer");
    if (kdbplan::SubmitCutter::check_ends(offs, nreads, nbytes) != kdbplan::SUBMIT_OK) return fail(KDB_ERR_ARG, "%s", kdbplan::SUBMIT_ENDS_TEXT);
    DeviceGuard g(e->device);
    HostFeed &f = e->feed;
    int rc = f.ensure_staging(e->k);
    if (rc != KDB_OK) return rc;
    if (src_pinned) {
        Event &ev = f.pin.ev[f.pin.idx];             // holds the event of call N-2
        if (!ev) HIP_TRY(ev.create());
        if (f.pin.used[f.pin.idx]) HIP_TRY(hipEventSynchronize(ev));
    }
    kdbplan::SubmitCutter cut(offs, nreads, first_continues, f.stage_bytes, f.stage_reads, e->k);
    while (!cut.done()) {
        StageSlot &s = f.stage[f.next_buf];
        if (s.inflight) { HIP_TRY(hipEventSynchronize(s.busy)); s.inflight = false; }
        uint8_t *hb = s.h_bases;
        uint64_t *ho = s.h_offs;
        kdbplan::SubmitPiece p;
        if (cut.next(ho, p) != kdbplan::SUBMIT_OK) return fail(KDB_ERR_ARG, kdbplan::SUBMIT_RISE_FORMAT, cut.bad);
        const uint64_t nb = p.nbytes;
        const size_t nr = p.nrecs;
        if (f.appends(p)) {
            if (f.acc_nb + nb > f.acc_cap || f.acc_nr + nr > f.acc_reads_cap) { rc = flush_accumulated(e); if (rc != KDB_OK) return rc; }
            AccSlot &a = f.acc[f.acc_slot];
            if (a.inflight) { HIP_TRY(hipEventSynchronize(a.ev_done)); a.inflight = false; }
            for (size_t i = 0; i <= nr; i++) ho[i] += f.acc_nb;                  // rebase onto the accumulated batch
            const uint8_t *src = src_pinned ? bases + p.start : hb;
            if (!src_pinned) parallel_copy(hb, bases + p.start, nb, e->copy_threads);
            HIP_TRY(hipMemcpyAsync(a.bases + f.acc_nb, src, nb, hipMemcpyHostToDevice, e->s_copy));
            // entries acc_nr .. acc_nr + nr of the offsets (entry acc_nr == acc_nb is rewritten with the same value)
            HIP_TRY(hipMemcpyAsync(a.offs + f.acc_nr, ho, (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->s_copy));
            HIP_TRY(hipEventRecord(s.ev_copied, e->s_copy));
            s.busy = s.ev_copied;                                                // staging is free once the copies are done
            f.acc_nb += nb; f.acc_nr += nr;
        } else {
            rc = flush_accumulated(e);                                             // keep the two paths from interleaving on a buffer
            if (rc != KDB_OK) return rc;
            if (src_pinned) {
                HIP_TRY(hipMemcpyAsync(s.d_bases, bases + p.start, nb, hipMemcpyHostToDevice, e->s_copy));
            } else {
                parallel_copy(hb, bases + p.start, nb, e->copy_threads);
                HIP_TRY(hipMemcpyAsync(s.d_bases, hb, nb, hipMemcpyHostToDevice, e->s_copy));
            }
            HIP_TRY(hipMemcpyAsync(s.d_offs, ho, (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->s_copy));
            HIP_TRY(hipEventRecord(s.ev_copied, e->s_copy));
            HIP_TRY(hipStreamWaitEvent(e->s_compute, s.ev_copied, 0));
            rc = launch_batch(e, s.d_bases, nb, s.d_offs, nr, p.first_is_continuation ? 1 : 0, BATCH_HOST_FED);
            if (rc != KDB_OK) return rc;
            HIP_TRY(hipEventRecord(s.ev_done, e->s_compute));
            s.busy = s.ev_done;
        }
        s.inflight = true;
        f.next_buf = (f.next_buf + 1) % NBUF;
    }
    if (src_pinned) {
        HIP_TRY(hipEventRecord(f.pin.ev[f.pin.idx], e->s_copy));
        f.pin.used[f.pin.idx] = true;
        f.pin.idx ^= 1;
    }
    return KDB_OK;
}

int kdb_submit(kdb_engine *e, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads) { return submit_impl(e, bases, nbytes, offs, nreads, false); }

int kdb_submit_pinned(kdb_engine *e, const uint8_t *bases, size_t nbytes, const uint64_t *offs, size_t nreads) { return submit_impl(e, bases, nbytes, offs, nreads, true); }

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
    e->feed.idle();
    if (e->prof) { int rc = prof_collect(e); if (rc != KDB_OK) return rc; }
#ifdef KDB_SC_PROF
    kdb::sc_prof_report();
#endif
    return check_errors(e);
}

// kdb_finish (emitted: Sum(counts) must be what the kernels emitted, and is then the total) and kdb_table_stats
static int read_vector(kdb_engine *e, uint64_t *counts_out, bool emitted, uint64_t *sum_out, uint64_t *unique_out)
{
    return engine_call(e, NEEDS_VECTOR | SYNCS_FIRST, [&]() -> int {
        kdb::DevCounters c;
        const int rc = vector_stats(e, e->d_table, counts_out, &c, emitted, [&] { stats_sweep(e, e->d_table); });
        if (rc != KDB_OK) return rc;
        if (sum_out) *sum_out = c.sum;
        if (unique_out) *unique_out = c.unique;
        return KDB_OK;
    });
}

int kdb_finish(kdb_engine *e, uint64_t *counts_out, uint64_t *total_kmers, uint64_t *unique_kmers) { return read_vector(e, counts_out, true, total_kmers, unique_kmers); }

int kdb_table_stats(kdb_engine *e, uint64_t *counts_out, uint64_t *sum_out, uint64_t *unique_out) { return read_vector(e, counts_out, false, sum_out, unique_out); }

int kdb_nullomers(kdb_engine *e, int folded, uint64_t *ids_out, uint64_t cap, uint64_t *n_out)
{
    return engine_call(e, NEEDS_VECTOR | SYNCS_FIRST,
                       [&]() -> int { return folded && !e->d_acc_table ? fail(KDB_ERR_STATE, "kdb_nullomers(folded) before any kdb_fold_file") : KDB_OK; },
                       [&] { return nullomers(e, folded ? e->d_acc_table.p : e->d_table, ids_out, cap, n_out); });
}

int kdb_reduce(kdb_engine *const *engines, int n, int root)
{
    if (!engines || n < 2 || n > KDB_REDUCE_MAX) return fail(KDB_ERR_ARG, "kdb_reduce: n=%d engines (2..%d)", n, KDB_REDUCE_MAX);
    if (root < 0 || root >= n) return fail(KDB_ERR_ARG, "kdb_reduce: root=%d of %d", root, n);
    for (int j = 0; j < n; j++) {
        kdb_engine *e = engines[j];
        if (!e) return fail(KDB_ERR_ARG, "kdb_reduce: engine %d is NULL", j);
        if (e->tableless) return fail(KDB_ERR_STATE, "kdb_reduce: engine %d was %s", j, NO_VECTOR);
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
    auto refusals = [&]() -> int {
        if (e->tableless || acc->tableless) return no_vector();
        if (e->k != acc->k || e->device != acc->device) return fail(KDB_ERR_ARG, "kdb_fold_file_into: the engines differ in k or device");
        return KDB_OK;
    };
    return engine_call(e, SYNCS_FIRST, refusals, [&]() -> int {
        if (((uintptr_t)e->d_table & 15u) != 0) return fail(KDB_ERR_ARG, "the count vector must be 16-byte aligned for kdb_fold_file");
        if (!acc->d_acc_table) {
            hipError_t me = acc->d_acc_table.alloc(acc->nbins * 8ull);
            if (me != hipSuccess) { (void)hipGetLastError(); return fail(KDB_ERR_NOMEM, "no room for a second 4^%d vector (accumulator): %s", e->k, hipGetErrorString(me)); }
            HIP_TRY(hipMemsetAsync(acc->d_acc_table, 0, acc->nbins * 8ull, e->s_compute));     // (ordered before this fold; later folds start after it has finished)
        }
        kdb::DevCounters c;
        const int rc = vector_stats(e, e->d_table, nullptr, &c, true, [&] {
            unsigned grid = (unsigned)((e->nbins / 2 + 255) / 256);
            if (grid > 256u * 16u) grid = 256u * 16u;
            if (grid == 0) grid = 1;
            hipLaunchKernelGGL(kdb::fold_kernel, dim3(grid), dim3(256), 0, e->s_compute, e->d_table, acc->d_acc_table.p, e->nbins, e->d_ctr.p);
        });
        if (rc != KDB_OK) return rc;
        if (total_kmers) *total_kmers = c.total_kmers;
        if (unique_kmers) *unique_kmers = c.unique;
        acc->folded_files++;
        acc->folded_total += c.total_kmers;
        // the file vector is all zero again: a new file starts (what kdb_reset does, without a second sweep of the vector)
        HIP_TRY(hipMemsetAsync(&e->d_ctr->total_kmers, 0, sizeof(unsigned long long), e->s_compute));
        HIP_TRY(hipStreamSynchronize(e->s_compute));
        e->tp.table_is_zero = e->owns_table && !e->table_escaped;
        return KDB_OK;
    });
}

int kdb_finish_folded(kdb_engine *e, uint64_t *counts_out, uint64_t *total_kmers, uint64_t *unique_kmers)
{
    return engine_call(e, SYNCS_FIRST, [&]() -> int { return e->d_acc_table ? KDB_OK : fail(KDB_ERR_STATE, "kdb_finish_folded before any kdb_fold_file"); }, [&]() -> int {
        kdb::DevCounters c;
        const int rc = vector_stats(e, e->d_acc_table, counts_out, &c, false, [&] { stats_sweep(e, e->d_acc_table); });
        if (rc != KDB_OK) return rc;
        if (c.sum != e->folded_total)
            return fail(KDB_ERR_STATE, "internal: Sum(accumulated counts)=%llu but the folded files held %llu k-mers", c.sum, (unsigned long long)e->folded_total);
        if (total_kmers) *total_kmers = c.sum;
        if (unique_kmers) *unique_kmers = c.unique;
        return KDB_OK;
    });
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
    return engine_call(e, 0, [&]() -> int {
        { int rc = flush_accumulated(e); if (rc != KDB_OK) return rc; }
        HIP_TRY(hipStreamSynchronize(e->s_compute));
        kdb::DevCounters c;
        HIP_TRY(hipMemcpy(&c, e->d_ctr, sizeof c, hipMemcpyDeviceToHost));
        if (n_short) *n_short = c.n_short;
        if (n_bad) *n_bad = c.n_bad;
        return KDB_OK;
    });
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
    std::vector<unsigned long long> ids(nbytes);
    const int rc = window_ids_run(e, seq, nbytes, nullptr, 1, ids.data());
    if (rc != KDB_OK) return rc;
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
    return window_ids_run(e, bases, nbytes, offs, nreads, (unsigned long long *)ids_out);
}

int kdb_copy_back_and_write_kdb_rows(kdb_engine *e, int folded, uint64_t *counts_out, const char *path, uint64_t total_kmers, int compresslevel,
                                     int nthreads, int encoder, uint64_t *nblocks_out)
{
    if (!e || !counts_out || !path) return fail(KDB_ERR_ARG, "NULL argument");
    auto refusals = [&]() -> int {
        if (folded && !e->d_acc_table) return fail(KDB_ERR_STATE, "kdb_copy_back_and_write_kdb_rows(folded) before any kdb_fold_file");
        if (encoder != KDB_ENCODER_DEFAULT && encoder != KDB_ENCODER_ROWS && encoder != KDB_ENCODER_ZLIB)
            return fail(KDB_ERR_ARG, "kdb_copy_back_and_write_kdb_rows: unknown encoder %d", encoder);
        return KDB_OK;
    };
    return engine_call(e, NEEDS_VECTOR | SYNCS_FIRST, refusals, [&]() -> int {
        const unsigned long long *vec = folded ? e->d_acc_table.p : e->d_table;
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
    });
}

int kdb_prof_enable(kdb_engine *e, int on)
{
    if (!e) return fail(KDB_ERR_ARG, "engine is NULL");
    e->prof = on != 0;
    return KDB_OK;
}

int kdb_prof_reset(kdb_engine *e)
{
    const int rc = kdb_prof_get(e, 0, nullptr, nullptr);           // (collects the spans still in flight)
    if (rc == KDB_OK) for (int i = 0; i < KDB_N_KERNELS; i++) { e->prof_ms[i] = 0; e->prof_n[i] = 0; }
    return rc;
}

int kdb_prof_get(kdb_engine *e, int kernel_id, double *total_ms, uint64_t *launches)
{
    return engine_call(e, 0, [&]() -> int { return kernel_id < 0 || kernel_id >= KDB_N_KERNELS ? fail(KDB_ERR_ARG, "kernel_id=%d", kernel_id) : KDB_OK; }, [&]() -> int {
        HIP_TRY(hipStreamSynchronize(e->s_compute));
        int rc = prof_collect(e);
        if (rc != KDB_OK) return rc;
        if (total_ms) *total_ms = e->prof_ms[kernel_id];
        if (launches) *launches = e->prof_n[kernel_id];
        return KDB_OK;
    });
}

}  // extern "C"

// the analysis calls, which take finished vectors and no engine (here, behind the engine: their kernel templates are instantiated last)
#include "kdb_analysis_host.hip.h"
