// kdb_scatter_host.hip.h -- the host side of the "paged scatter" paths (kernels: kdb_scatter.hip.h): what sizes, allocates for and
// launches them.  Options (PagedOptions) are the engine's and are only read here; the structs below hold device pointers, capacities
// and bookkeeping.
#pragma once
#include "kdb_scatter.hip.h"

namespace kdb {

// k = 13 in ONE level: 26 id bits = 10 bucket bits + 16 bin bits.  1024 rings of 64 u16 elements (128 KiB of LDS) leave room for
// one workgroup per CU, so that workgroup has 1024 threads (16 waves per CU, as two workgroups of 512 have) and a tile of 1023
// chunks; a bucket's 65536 bins share the 32768 histogram words as two 16-bit counters each (page_hist_kernel<true>, as at
// k = 17).  Level 2 of the two-level path existed at k = 13 only to split one more bit pair: 4.48 -> see DESIGN.md section 5.
constexpr int SC1_THREADS = 1024, SC1_RINGS = 1024, SC1_GRID = 256, SC1_K = 13;

// tuning options of the paged paths (engine options of the same meaning: kdb_engine_options.hip.h, the option table)
struct PagedOptions {
    int grid = 0;                          // persistent workgroups (0 = SC_GRID)
    int lo_bits = 0;                       // id bits below the bucket field; 0 = SC_LO_BITS_ONE_LEVEL / _TWO_LEVEL (SC_LO_BITS_MAX: buckets from the leading id bits, uneven in canonical mode)
    int contig_pages = 1;                  // 1: workgroup w's pages are w * wg_pages + p (level 1 at k = 15: 2.26 -> 2.18 ms), 0: w + p * G
    int wide_lines = 1;                    // 1: k <= 12 writes its pages in 128-byte pieces (engine option sc_wide_lines)
    int l1_wide = 1;                       // 1: level 1 writes its pages in 128-byte pieces, one workgroup of 1024 threads per CU (engine option l1_wide_lines)
    int l2_wide = 1;                       // 1: level 2 writes its pages in 128-byte pieces, one workgroup of 1024 threads per CU (engine option l2_wide_lines)
    int l1_one_round = 1;                  // 1: level 1 of k <= 15 (<= 64 leading digits) with 128 rings of 256 elements: one placement round per tile (engine option l1_one_round)
    int l1k = 1;                           // 1: k = 15 (canonical, DROP) runs level 1's kernel compiled for that k; 0: the generic one (comparison)
    int one_level_max_k = SC1_K;           // largest k counted with one scatter level (13: the 1024-ring kernel; 12: k = 13 takes the two-level path, for comparison)
    int defer = 1;                         // 1: the histogram pass over the arena waits for as many batches as fit
    size_t budget_bytes = 0;               // arena size; 0 = decide at first use (85 % of the free memory, less reserve_bytes: TwoLevelPaged::budget_decided)
    size_t reserve_bytes = 0;              // device memory the arena must leave free whatever it grows to (RCCL's buffers and the reduce's scratch: kmerdb_amd/distributed.py)
    int grow = 1;                          // 0: the arena keeps its first size; 1: it doubles when that pays (arena_room); 2: whenever it has filled up
    int first_batches = 8;                 // the arena's first size, in batches like the first one (engine option arena_batches)
    int one_level_defer = -1;              // the one-level path (k = 9 .. one_level_max_k): 0 = sort and histogram pass per batch; N >= 2 = once per N scattered batches
                                           // (OneLevelPending); -1 = ONE_LEVEL_DEPTH for k <= 12, 0 for k = 13 (one_level_depth)
};
// Depth 4 takes 85 % of what depth 8 takes off the k = 12 headline step (-0.095 of 1.85 ms against -0.11; depth 2: -0.08) for half the arena, 12 GB for batches of
// 10 M reads of 150 bases (profiles/one_level_defer_ab.txt).  k = 13 in one level keeps the immediate path unless asked: not measured.
constexpr int ONE_LEVEL_DEPTH = 4;
inline int one_level_depth(const PagedOptions &opt, int k) { return opt.one_level_defer >= 0 ? opt.one_level_defer : (k <= 12 ? ONE_LEVEL_DEPTH : 0); }

// shared by every path: a set of pages, the sort of its tags, the histogram pass, the sizing of a sub-batch, the scatter kernels' launch
// a set of pages with their tags, the page list that the sort of the tags makes, and the bucket arrays of that sort:
// the scratch of the one-level path, of level 1, and the arena
struct ScatterState {
    uint8_t *pages = nullptr; size_t cap = 0, page_bytes = 0;   // in pages of page_bytes
    uint32_t *tag = nullptr;                                    // [cap]
    PageEntry *list = nullptr;                                  // [cap]
    uint32_t *d_bkt = nullptr; size_t bkt_cap = 0;              // bkt_arrays for bkt_cap buckets
    // What a page sort starts from -- unused pages' tags say "no page", bucket counts are zero -- is also what it leaves behind (the place kernel
    // restores the tags it reads, the scan zeroes the counts), so the memsets run only for what is not known to be clean:
    size_t tags_dirty = 0;                                      // tags [0, tags_dirty) may hold something else: a new page set, pages written but never sorted
    size_t bkt_zero_nb = 0;                                     // bkt_pages and bkt_elems are zero as laid out for this many buckets (0: not known)
};

inline void page_set_free(ScatterState &st)
{
    if (st.pages) (void)hipFree(st.pages);
    if (st.tag) (void)hipFree(st.tag);
    if (st.list) (void)hipFree(st.list);
    st.pages = nullptr; st.tag = nullptr; st.list = nullptr; st.cap = 0; st.tags_dirty = 0;
}

// pages, tags and list for npages; 0 ok, 2 no room (no page set is held then); the old set must have been freed
inline int page_set_alloc(ScatterState &st, size_t npages, size_t page_bytes)
{
    if (hipMalloc((void **)&st.pages, npages * page_bytes) == hipSuccess && hipMalloc((void **)&st.tag, npages * sizeof(uint32_t)) == hipSuccess &&
        hipMalloc((void **)&st.list, npages * sizeof(PageEntry)) == hipSuccess) { st.cap = npages; st.page_bytes = page_bytes; st.tags_dirty = npages; return 0; }
    (void)hipGetLastError();
    page_set_free(st);
    return 2;
}

inline void scatter_free(ScatterState &st)
{
    page_set_free(st);
    if (st.d_bkt) (void)hipFree(st.d_bkt);
    st = ScatterState();
}

// the bucket arrays, one allocation: bkt_pages [nb] | bkt_elems [nb] | page_base [nb + 1] | slice_base [nb + 1] | and, for the direct form of
// the sort (nb <= PAGES_DIRECT_NB), wg_off [PAGES_DIRECT_GRID][nb]
struct BktArrays { uint32_t *pages, *elems, *page_base, *slice_base, *wg_off; };
inline BktArrays bkt_arrays(const ScatterState &st, size_t nb) { return {st.d_bkt, st.d_bkt + nb, st.d_bkt + 2 * nb, st.d_bkt + 3 * nb + 1, st.d_bkt + 4 * nb + 2}; }
inline size_t bkt_words(size_t nb) { return 4 * nb + 2 + (nb <= (size_t)PAGES_DIRECT_NB ? (size_t)PAGES_DIRECT_GRID * nb : 0); }

inline int reserve_error(int rc) { if (rc) partition_error_ref() = rc == 2 ? "scratch allocation failed" : "stream error"; return rc; }

// room for nb buckets; 0 ok, 1 stream error, 2 no room
inline int bkt_reserve(ScatterState &st, hipStream_t stream, size_t nb)
{
    if (st.bkt_cap >= nb) return 0;
    if (st.d_bkt) { if (hipStreamSynchronize(stream) != hipSuccess) return reserve_error(1); (void)hipFree(st.d_bkt); st.d_bkt = nullptr; st.bkt_cap = 0; }
    st.bkt_zero_nb = 0;
    size_t words = bkt_words(nb);          // (room for every layout of up to nb buckets: the direct form's is largest at PAGES_DIRECT_NB)
    if (nb > (size_t)PAGES_DIRECT_NB && words < bkt_words((size_t)PAGES_DIRECT_NB)) words = bkt_words((size_t)PAGES_DIRECT_NB);
    if (hipMalloc((void **)&st.d_bkt, words * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); return reserve_error(2); }
    st.bkt_cap = nb;
    return 0;
}

// room for npages pages of page_bytes and nb buckets; 0 ok, 1 stream error, 2 no room
inline int scatter_reserve(ScatterState &st, hipStream_t stream, size_t npages, size_t nb, size_t page_bytes = SC_PAGE_BYTES)
{
    if (st.cap < npages || st.page_bytes != page_bytes) {
        if (st.pages) { if (hipStreamSynchronize(stream) != hipSuccess) return reserve_error(1); page_set_free(st); }
        if (page_set_alloc(st, npages, page_bytes)) return reserve_error(2);
    }
    return bkt_reserve(st, stream, nb);
}

// before pages of `st` are written: the tags not known to say "no page" are cleared (a new page set; pages written and dropped before a sort read them)
inline int tags_clean(ScatterState &st, hipStream_t stream)
{
    if (st.tags_dirty > st.cap) st.tags_dirty = st.cap;
    if (st.tags_dirty && hipMemsetAsync(st.tag, 0xFF, st.tags_dirty * sizeof(uint32_t), stream) != hipSuccess) { partition_error_ref() = "memset failed"; return 1; }
    st.tags_dirty = 0;
    return 0;
}

// the page sort: a counting sort of the first `npages` tags into one page list per bucket, histogram slices of `slice_pages` pages.
// It leaves those tags saying "no page" and the bucket counts zero (kdb_scatter.hip.h); the counts are cleared here where that is not known.
inline int page_sort(hipStream_t stream, ScatterState &st, uint32_t npages, uint32_t nb, unsigned long long *stat, uint32_t line_elems, uint32_t slice_pages,
                     uint32_t grid_cap, DevCounters *scan_ctr)
{
    const BktArrays b = bkt_arrays(st, nb);
    if (st.bkt_zero_nb != nb) {
        st.bkt_zero_nb = 0;
        if (hipMemsetAsync(st.d_bkt, 0, 2 * (size_t)nb * sizeof(uint32_t), stream) != hipSuccess) { partition_error_ref() = "memset failed"; return 1; }
    }
    const bool direct = nb <= (uint32_t)PAGES_DIRECT_NB;
    if (direct && grid_cap > (uint32_t)PAGES_DIRECT_GRID) grid_cap = (uint32_t)PAGES_DIRECT_GRID;
    const uint32_t pgrid = (npages + 4095u) / 4096u < grid_cap ? (npages + 4095u) / 4096u : grid_cap;
    const auto count = direct ? pages_count_kernel<false> : pages_count_kernel<true>;
    const auto place = direct ? pages_place_kernel<false> : pages_place_kernel<true>;
    hipLaunchKernelGGL(count, dim3(pgrid), dim3(PAGES_THREADS), 0, stream, (const uint32_t *)st.tag, npages, nb, b.pages, b.elems, b.wg_off, stat, line_elems);
    hipLaunchKernelGGL(pages_scan_kernel, dim3(1), dim3(1024), 0, stream, b.pages, b.elems, nb, b.page_base, b.slice_base, slice_pages, direct ? 1 : 0, scan_ctr);
    hipLaunchKernelGGL(place, dim3(pgrid), dim3(PAGES_THREADS), 0, stream, st.tag, npages, nb, b.pages, (const uint32_t *)b.page_base, (const uint32_t *)b.wg_off, st.list);
    if (hipPeekAtLastError() == hipSuccess) {
        st.bkt_zero_nb = nb;
        if (st.tags_dirty <= npages) st.tags_dirty = 0;
    }
    return 0;
}

// the histogram pass over sorted pages: a workgroup per slice of a bucket's list (bins16: two 16-bit counters per histogram word)
inline void hist_pass(hipStream_t stream, bool bins16, const ScatterState &st, uint32_t npages, uint32_t nb, uint32_t slice_pages, unsigned long long *d_table, int lo_bits,
                      int hi_shift, int table_is_zero, DevCounters *d_ctr)
{
    const BktArrays b = bkt_arrays(st, nb);
    const uint32_t p2_grid = npages / slice_pages + nb + 1u;
    const auto fn = bins16 ? page_hist_kernel<true> : page_hist_kernel<false>;
    hipLaunchKernelGGL(fn, dim3(p2_grid), dim3(P2_THREADS), 0, stream, (const uint8_t *)st.pages,
                       (const PageEntry *)st.list, (const uint32_t *)b.page_base, (const uint32_t *)b.slice_base, nb, d_table, lo_bits, hi_shift, table_is_zero, d_ctr);
}

// tiles per launch: sub-batches of 2 Gi positions (page numbers stay well inside 32 bits), and fewer than 4096 tiles per
// workgroup (a thread's packed 16 + 16-bit statistics of <= 16 per tile cannot carry)
inline uint64_t scatter_max_tiles(uint32_t Gmax, uint32_t tile_pos = SC_TILE_POS)
{
    const uint64_t a = (1ull << 31) / tile_pos, b = 4095ull * Gmax;
    return a < b ? a : b;
}

// what the sizing of a sub-batch rests on: the tiles of the batch and the rings and pages of the kernel that scatters them
struct TileGeom {
    int rings;
    uint32_t tile_pos, Gmax, page_elems;
    uint64_t ntiles_all, max_tiles;
};

inline void tile_geometry(TileGeom &g, size_t nbytes, uint32_t tile_stride, uint32_t Gmax)
{
    g.tile_pos = tile_stride * 16u;
    g.ntiles_all = ((nbytes + 15) / 16 + tile_stride - 1) / tile_stride;
    g.Gmax = Gmax;
    g.max_tiles = scatter_max_tiles(Gmax, g.tile_pos);
}

// the sub-batch that begins at tile t0 (t0 = 0: the largest of the batch, which the scratch is reserved for)
struct ScLaunch { uint32_t nt, G, extra_elems, wg_pages, npages; };

inline ScLaunch sub_batch(const TileGeom &g, uint64_t t0, int n_expand)
{
    ScLaunch L;
    L.nt = (uint32_t)((g.ntiles_all - t0) < g.max_tiles ? (g.ntiles_all - t0) : g.max_tiles);
    L.G = L.nt < g.Gmax ? L.nt : g.Gmax;
    const uint64_t wg_pos = (uint64_t)((L.nt + L.G - 1) / L.G) * g.tile_pos;          // window positions of a workgroup's tiles
    // EXPAND mode: fills of N-windows (4 or 16 per window) go through the rings like every other id; a workgroup's page sequence has
    // room for half as many of them as it has window positions (0.5 % N at k = 12 makes a quarter), at least one full pass of
    // 16 per thread; beyond that a workgroup adds its fills to the vector directly
    const uint64_t floor_ = 16u * 1024u + 1024u * 64u + 2048u;                           // (a round of 1024 threads, what the rings hold, slack)
    const uint64_t extra = !n_expand ? 0 : (wg_pos / 2 > floor_ ? wg_pos / 2 : floor_);
    L.extra_elems = (uint32_t)(extra < 0x7FFFFFFFull ? extra : 0x7FFFFFFFull);
    // pages a workgroup can need: every element it can emit, one partial page per ring, one spare
    L.wg_pages = (uint32_t)((wg_pos + L.extra_elems + g.page_elems - 1) / g.page_elems) + (uint32_t)g.rings + 1u;
    L.npages = L.G * L.wg_pages;
    return L;
}

using BasesKernel = void (*)(const uint8_t *, uint64_t, uint32_t, uint32_t, int, int, int, int, ScOut, unsigned long long *, DevCounters *, RecStarts);
using IdsKernel = void (*)(const uint8_t *, const PageEntry *, const uint32_t *, uint32_t, int, int, ScOut, DevCounters *);
// scatter_bases_kernel is launched as a pair: only the device knows whether a batch's records are of one length, and the form that does not apply returns at once
struct BasesPair { BasesKernel fn[2] /* for records of one length, for ragged ones */; int threads; };

template <typename ID, typename EL, int RG, int CC, int RD, int TH, bool E, bool CN, int KK = 0>
inline BasesPair bases_pair() { return {{scatter_bases_kernel<ID, EL, RG, CC, RD, E, CN, KK, TH, false>, scatter_bases_kernel<ID, EL, RG, CC, RD, E, CN, KK, TH, true>}, TH}; }

template <typename ID, typename EL, int RG, int CC, int RD, int TH, int KK = 0>
inline BasesPair bases_modes(int n_expand, int canonical)
{
    if (n_expand) return canonical ? bases_pair<ID, EL, RG, CC, RD, TH, true, true, KK>() : bases_pair<ID, EL, RG, CC, RD, TH, true, false, KK>();
    return canonical ? bases_pair<ID, EL, RG, CC, RD, TH, false, true, KK>() : bases_pair<ID, EL, RG, CC, RD, TH, false, false, KK>();
}

// the batch in hand and where its counts go
struct ScBatch {
    const uint8_t *d_bases; size_t nbytes; RecStarts rs;
    int k, canonical, n_expand;
    unsigned long long *d_table; DevCounters *d_ctr;
};

// sub-batch L through a scatter_bases_kernel pair into the pages of `st`, whose tags say "no page": the sort of the sub-batch before left them so,
// and tags_clean sees to the rest
// (region >= 0: into the L.npages pages of `st` that begin at page `region` -- the kernels number their pages from the pointers they are given --;
//  the deferred one-level path looks after the tags itself, once per cycle)
inline int launch_bases(const BasesPair &kp, hipStream_t stream, ProfHook &prof, ScatterState &st, const ScLaunch &L, int contig_pages,
                        const ScBatch &B, uint64_t t0, int ring_shift, int ring_bits, int sub_log2, int64_t region = -1)
{
    ScOut out;
    out.pages = st.pages; out.tag = st.tag; out.extra_elems = L.extra_elems; out.wg_pages = L.wg_pages;
    out.wg_range = nullptr; out.contig = (uint32_t)contig_pages; out.wg_base = 0; out.grid = 0;
    if (region >= 0) { out.pages += (size_t)region * st.page_bytes; out.tag += (size_t)region; }
    else {
        if (tags_clean(st, stream)) return 1;
        st.tags_dirty = L.npages;                                        // (until the sort has read them)
    }
    prof.begin_on(KDB_KERNEL_SCATTER, stream);
    for (BasesKernel fn : kp.fn)
        hipLaunchKernelGGL(fn, dim3(L.G), dim3(kp.threads), 0, stream, B.d_bases, (uint64_t)B.nbytes, (uint32_t)t0, L.nt, B.k, ring_shift, ring_bits, sub_log2, out,
                           B.d_table, B.d_ctr, B.rs);
    prof.end();
    return 0;
}

// ---------------------------------------------------------------------------------
// host: 8 <= k <= 12 (and k = 13 in one level)
// ---------------------------------------------------------------------------------
// The one-level path in two stages, so that they can run on different streams: stage 1 = the scatter kernel of a sub-batch into the
// pages of `st`, stage 2 = the page sort and the histogram pass over those pages.  ScGeom: what the host works out once per batch.
struct ScGeom : TileGeom {
    bool big; bool wide /* k <= 12 in 128-byte pieces: one workgroup of 1024 threads per CU, 512 rings of 128 elements (u16w) */;
    int binb, nb, sub_log2, nb_bits, lo_bits, hi_shift;
};

inline ScGeom scatter_geometry(const PagedOptions &opt, size_t nbytes, int k, uint32_t grid_default = 0)
{
    ScGeom g;
    g.big = k == SC1_K;                                                  // 1024 threads, 1024 rings, 16-bit bins
    g.binb = g.big ? 16 : BIN_BITS;
    g.nb = 1 << (2 * k - g.binb);                                        // buckets: 2 (k = 8) .. 512 (k = 12), 1024 (k = 13)
    g.rings = g.big ? SC1_RINGS : 512;
    g.page_elems = 512;
    g.lo_bits = opt.lo_bits ? opt.lo_bits : SC_LO_BITS_ONE_LEVEL;        // (lo_bits = 15: bucket = leading id bits, for comparison)
    g.wide = !g.big && opt.wide_lines != 0;
    g.sub_log2 = 0; g.nb_bits = 2 * k - g.binb;
    while ((g.nb << g.sub_log2) < g.rings) g.sub_log2++;                 // few buckets: each gets several rings (no same-address pile-up)
    g.hi_shift = g.lo_bits + g.nb_bits;
    tile_geometry(g, nbytes, (g.big || g.wide) ? (uint32_t)SC1_THREADS - 1u : (uint32_t)SC_TILE_STRIDE,
                  opt.grid > 0 ? (uint32_t)opt.grid : (grid_default ? grid_default : (uint32_t)((g.big || g.wide) ? SC1_GRID : SC_GRID)));
    return g;
}

inline BasesPair select_one_level(const ScGeom &g, int k, int n_expand, int canonical)
{
    if (g.big) {
        if (g.lo_bits == SC_LO_BITS_ONE_LEVEL) return bases_modes<uint32_t, uint16_t, SC1_RINGS, 64, 16, SC1_THREADS, SC1_K>(n_expand, canonical);      // shifts and masks compiled in
        return bases_modes<uint32_t, uint16_t, SC1_RINGS, 64, 16, SC1_THREADS>(n_expand, canonical);
    }
    if (g.wide) {
        // 128-byte pieces: one workgroup of 1024 threads per CU, 512 rings of 128 elements
        // (shifts, masks and rings per bucket compiled in for the default bucket field: two dozen scalar registers stay free)
        const bool compiled = g.lo_bits == SC_LO_BITS_ONE_LEVEL && (g.nb << g.sub_log2) == 512;
        if (compiled && k == 12) return bases_modes<uint32_t, u16w, 512, 128, 16, SC1_THREADS, 12>(n_expand, canonical);                                // BASELINE's headline k
        if (compiled && k == 11) return bases_modes<uint32_t, u16w, 512, 128, 16, SC1_THREADS, 11>(n_expand, canonical);
        if (compiled && k == 10) return bases_modes<uint32_t, u16w, 512, 128, 16, SC1_THREADS, 10>(n_expand, canonical);
        if (compiled && k == 9) return bases_modes<uint32_t, u16w, 512, 128, 16, SC1_THREADS, 9>(n_expand, canonical);
        return bases_modes<uint32_t, u16w, 512, 128, 16, SC1_THREADS>(n_expand, canonical);
    }
    if (k == 12 && g.lo_bits == SC_LO_BITS_ONE_LEVEL && g.sub_log2 == 0)
        return bases_modes<uint32_t, uint16_t, 512, 64, 16, SC_THREADS, 12>(n_expand, canonical);                 // ... in 64-byte lines, two workgroups per CU
    return bases_modes<uint32_t, uint16_t, 512, 64, 16, SC_THREADS>(n_expand, canonical);
}

inline int scatter_stage1(ScatterState &st, const PagedOptions &opt, hipStream_t stream, const ScGeom &g, uint64_t t0, const ScBatch &B, ProfHook &prof, ScLaunch *L)
{
    *L = sub_batch(g, t0, B.n_expand);
    if (launch_bases(select_one_level(g, B.k, B.n_expand, B.canonical), stream, prof, st, *L, opt.contig_pages, B, t0, g.lo_bits, g.nb_bits, g.sub_log2))
        return 1;
    if (hipGetLastError() != hipSuccess) { partition_error_ref() = "paged scatter failed to launch"; return 1; }
    return 0;
}

inline int scatter_stage2(ScatterState &st, hipStream_t stream, const ScGeom &g, const ScLaunch &L, const ScBatch &B, ProfHook &prof)
{
    const uint32_t target = 512u;                                    // P2 workgroups in all (fewer, larger slices win: single-slice buckets flush without atomics)
    const uint32_t est_pages = (uint32_t)(((uint64_t)L.nt * g.tile_pos * 2) / SC_PAGE_BYTES) + 1u;
    uint32_t slice_pages = (est_pages + target - 1) / target;
    if (slice_pages < 128u) slice_pages = 128u;                      // >= 64 Ki elements per histogram
    prof.begin_on(KDB_KERNEL_PAGE_SORT, stream);
    const int src = page_sort(stream, st, L.npages, (uint32_t)g.nb, &B.d_ctr->pages_bases, 32u, slice_pages, 256u, B.d_ctr);
    prof.end();
    if (src) return src;
    prof.begin_on(KDB_KERNEL_PAGE_HIST, stream);
    hist_pass(stream, g.big, st, L.npages, (uint32_t)g.nb, slice_pages, B.d_table, g.lo_bits, g.hi_shift, 0, B.d_ctr);
    prof.end();
    if (hipGetLastError() != hipSuccess) { partition_error_ref() = "paged scatter failed to launch"; return 1; }
    return 0;
}

// returns 0 ok, 1 error (partition_error()), 2 no room for the scratch (nothing was counted)
inline int scatter_count(ScatterState &st, const PagedOptions &opt, hipStream_t stream, const ScBatch &B, ProfHook &prof)
{
    const ScGeom g = scatter_geometry(opt, B.nbytes, B.k);
    { const int rc = scatter_reserve(st, stream, sub_batch(g, 0, B.n_expand).npages, (size_t)g.nb); if (rc) return rc; }      // (the largest sub-batch)
    for (uint64_t t0 = 0; t0 < g.ntiles_all; t0 += g.max_tiles) {
        ScLaunch L;
        if (scatter_stage1(st, opt, stream, g, t0, B, prof, &L)) return 1;
        if (scatter_stage2(st, stream, g, L, B, prof)) return 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------
// The one-level path with stage 2 DEFERRED (option one_level_defer = N >= 2).  Stage 2 has a price that does not depend on the batch: every
// workgroup of the pass locates its slice, zeroes 128 KiB of LDS and adds all 32768 counters of its bucket to the vector (a canonical engine
// stages forward ids, so every bin of the 4^k vector is touched: the whole vector is read and written once per pass), and the sort and the pass
// are four dependent dispatches behind two memsets.  None of that is needed while more batches are still to come: a batch's scatter kernel
// writes into a region of its own in an arena, behind the regions of the batches already pending, and ONE sort of all their tags and ONE pass
// add them to the vector -- when N batches are pending, when the next region does not fit, and at kdb_sync (which everything that reads the
// vector goes through).  Scatter kernels and passes still never run side by side, and additions commute: the vector after a flush is what the
// immediate path leaves, bit for bit.
// ---------------------------------------------------------------------------------
struct OneLevelPending {
    ScatterState arena;
    size_t used = 0;                       // pages of the regions handed out since the last flush: [0, used) is what the sort reads
    size_t est_pages = 0;                  // pages those batches are expected to have filled (sizes the pass's slices, as scatter_stage2 does for one batch)
    int pending = 0;                       // batches in the arena
    // what the pending batches were scattered under; a batch that differs in any of it flushes them first
    int k = 0, nb = 0, lo_bits = 0, hi_shift = 0; bool big = false;
    unsigned long long *d_table = nullptr; // where their counts go (the vector, or a canonical engine's staging vector of forward counts)
    size_t budget_decided = 0;             // the arena's budget where the option leaves it open, decided at first use (as TwoLevelPaged's)
    bool grow_failed = false;              // an arena of the wanted size could not be allocated: no further attempts to enlarge it
    uint64_t reallocs = 0, flushes = 0, flushed_batches = 0, full_flushes = 0;      // full_flushes: flushes because the next region did not fit
};
constexpr size_t ARENA_BYTES_PER_PAGE = SC_PAGE_BYTES + sizeof(uint32_t) + sizeof(PageEntry);      // a page, its tag, its list entry

inline void one_level_free(OneLevelPending &ol) { scatter_free(ol.arena); ol = OneLevelPending(); }

// kdb_reset / after a flush: no batch is pending any more.  A flush's sort has put the tags back to "no page"; tags that were written and are
// dropped unsorted are cleared when the next cycle begins (arena.tags_dirty).
inline void one_level_drop(OneLevelPending &ol, bool sorted = false)
{
    if (!sorted && ol.used > ol.arena.tags_dirty) ol.arena.tags_dirty = ol.used;
    ol.used = 0; ol.est_pages = 0; ol.pending = 0;
}

// pages a sub-batch is expected to fill: two bytes per window position
inline size_t one_level_est_pages(const ScGeom &g, const ScLaunch &L) { return (size_t)(((uint64_t)L.nt * g.tile_pos * 2) / SC_PAGE_BYTES) + 1u; }

// one sort of every pending tag, one histogram pass
inline int one_level_flush(OneLevelPending &ol, hipStream_t stream, DevCounters *d_ctr, ProfHook &prof)
{
    if (ol.used == 0) { one_level_drop(ol); return 0; }
    // slices from the pending total: 512 workgroups in all, as for one batch, so that buckets of uniform input stay single-slice and flush
    // without atomics; never 2^26 elements in a slice (the LDS counters are 32 bits wide, WRAP_MAX rests on it)
    const size_t target = 512;
    size_t slice_pages = (ol.est_pages + target - 1) / target;
    if (slice_pages < 128) slice_pages = 128;
    if (slice_pages > (1u << 17) - 1u) slice_pages = (1u << 17) - 1u;
    prof.begin_on(KDB_KERNEL_PAGE_SORT, stream);
    const int src = page_sort(stream, ol.arena, (uint32_t)ol.used, (uint32_t)ol.nb, &d_ctr->pages_bases, 32u, (uint32_t)slice_pages, 256u, d_ctr);
    prof.end();
    if (src) return src;
    prof.begin_on(KDB_KERNEL_PAGE_HIST, stream);
    hist_pass(stream, ol.big, ol.arena, (uint32_t)ol.used, (uint32_t)ol.nb, (uint32_t)slice_pages, ol.d_table, ol.lo_bits, ol.hi_shift, 0, d_ctr);
    prof.end();
    ol.flushes++; ol.flushed_batches += (uint64_t)ol.pending;
    one_level_drop(ol, ol.arena.tags_dirty == 0);
    if (hipGetLastError() != hipSuccess) { partition_error_ref() = "histogram pass over the one-level arena failed to launch"; return 1; }
    return 0;
}

// An arena that holds the region of `need` pages behind what is pending: flushes what is pending if the region does not fit, and (re)allocates
// where the arena is missing, too small for two such regions, or smaller than `depth` of them when it has just filled up.
// 0 ok, 1 error, 3 no room for two regions within the budget (nothing is pending then: the batch takes the immediate path)
inline int one_level_room(OneLevelPending &ol, const PagedOptions &opt, hipStream_t stream, int depth, size_t need, size_t nb, DevCounters *d_ctr, ProfHook &prof)
{
    if (ol.arena.cap && ol.used + need <= ol.arena.cap && ol.arena.bkt_cap >= nb) return 0;
    const bool filled_up = ol.used != 0;
    if (filled_up) { ol.full_flushes++; if (one_level_flush(ol, stream, d_ctr, prof)) return 1; }
    if (opt.budget_bytes == 0 && ol.budget_decided == 0) {
        // as the two-level arena: 85 % of what is free at first use, less what the caller reserved
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        ol.budget_decided = free_b / 100 * 85;
        if (opt.reserve_bytes && ol.budget_decided + opt.reserve_bytes > free_b) ol.budget_decided = free_b > opt.reserve_bytes ? free_b - opt.reserve_bytes : 0;
        if (ol.budget_decided > (192ull << 30)) ol.budget_decided = 192ull << 30;
        if (ol.budget_decided == 0) ol.budget_decided = 1;
    }
    size_t budget_pages = (opt.budget_bytes ? opt.budget_bytes : ol.budget_decided) / ARENA_BYTES_PER_PAGE;
    if (ol.grow_failed && budget_pages > ol.arena.cap) budget_pages = ol.arena.cap;
    size_t want = (size_t)depth * need;
    if (want > budget_pages) want = budget_pages;
    // a new arena if this one cannot hold two such regions, or if it has just filled up and one a quarter larger (at least) is wanted and allowed
    const bool too_small = ol.arena.cap < 2 * need, grow = filled_up && want >= ol.arena.cap + ol.arena.cap / 4;
    if (too_small || grow) {
        // (only where it is too small: a quarter more than two regions is more than two.  What was free is asked again next time.)
        if (want < 2 * need) { ol.budget_decided = 0; return 3; }
        if (hipStreamSynchronize(stream) != hipSuccess) return reserve_error(1);
        page_set_free(ol.arena);
        ol.reallocs++;
        if (page_set_alloc(ol.arena, want, SC_PAGE_BYTES) != 0) {
            ol.grow_failed = true;                                      // (what could be had is the budget from now on)
            if (page_set_alloc(ol.arena, 2 * need, SC_PAGE_BYTES) != 0) return 3;
        }
    }
    const int rc = bkt_reserve(ol.arena, stream, nb);
    return rc == 2 ? 3 : rc;
}

// the tags a cycle begins with say "no page": after a flush they do, and nothing is cleared
inline int one_level_begin_cycle(OneLevelPending &ol, hipStream_t stream) { return tags_clean(ol.arena, stream); }

// returns 0 ok (the batch is scattered; its counts reach the vector with the next flush), 1 error (partition_error()),
// 3 no room for an arena of two regions (nothing of the batch was counted and nothing is pending): count it with scatter_count
inline int scatter_count_deferred(OneLevelPending &ol, const PagedOptions &opt, hipStream_t stream, const ScBatch &B, ProfHook &prof)
{
    const ScGeom g = scatter_geometry(opt, B.nbytes, B.k);
    const int depth = one_level_depth(opt, B.k);
    if (ol.used && (ol.k != B.k || ol.nb != g.nb || ol.lo_bits != g.lo_bits || ol.hi_shift != g.hi_shift || ol.big != g.big || ol.d_table != B.d_table)) {
        if (one_level_flush(ol, stream, B.d_ctr, prof)) return 1;
    }
    { const int rc = one_level_room(ol, opt, stream, depth, sub_batch(g, 0, B.n_expand).npages, (size_t)g.nb, B.d_ctr, prof); if (rc) return rc; }      // (the largest sub-batch)
    ol.k = B.k; ol.nb = g.nb; ol.lo_bits = g.lo_bits; ol.hi_shift = g.hi_shift; ol.big = g.big; ol.d_table = B.d_table;
    const BasesPair kp = select_one_level(g, B.k, B.n_expand, B.canonical);
    for (uint64_t t0 = 0; t0 < g.ntiles_all; t0 += g.max_tiles) {
        const ScLaunch L = sub_batch(g, t0, B.n_expand);
        // (a later sub-batch of a batch of more than 2 Gi positions: the arena holds two of the largest, so after a flush it fits)
        if (ol.used + L.npages > ol.arena.cap) { ol.full_flushes++; if (one_level_flush(ol, stream, B.d_ctr, prof)) return 1; }
        if (ol.used == 0 && one_level_begin_cycle(ol, stream)) return 1;
        if (launch_bases(kp, stream, prof, ol.arena, L, opt.contig_pages, B, t0, g.lo_bits, g.nb_bits, g.sub_log2, (int64_t)ol.used)) return 1;
        if (hipGetLastError() != hipSuccess) { partition_error_ref() = "paged scatter failed to launch"; return 1; }
        ol.used += L.npages;
        ol.est_pages += one_level_est_pages(g, L);
    }
    ol.pending++;
    if (ol.pending >= depth) return one_level_flush(ol, stream, B.d_ctr, prof);
    return 0;
}

// ---------------------------------------------------------------------------------
// The one-level path with the two stages of CONSECUTIVE batches side by side: the scatter kernel is bound by
// VALU issue, the histogram pass by HBM and LDS atomics, and on one stream they take turns.  Two sets of pages; batch i's stage 2 runs
// on a second stream while batch i + 1's stage 1 runs on the first.  The histogram passes stay in order (one stream: their plain
// read-modify-writes of the vector never meet each other), and a scatter kernel that runs beside a pass leaves its degenerate ids in
// a side list (hot_add) that is added behind the pass of its own batch.  DROP mode and batches of one sub-batch only (the callers fall
// back to scatter_count otherwise).  CU masks on the two streams (hipExtStreamCreateWithCUMask) give each stage its own CUs: both stages
// want most of a CU's LDS, so without masks a pass only finds room where the scatter kernel's persistent workgroups have ended.
// ---------------------------------------------------------------------------------
struct OverlapState {
    ScatterState sc[2];
    unsigned long long *side[2] = {nullptr, nullptr};
    size_t side_cap = 0;                                                  // pairs
    hipEvent_t scattered[2] = {nullptr, nullptr}, hist_done[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int next = 0, last = -1;                                              // set of the next batch; set whose pass was launched last (-1: none outstanding)
    uint32_t grid = 0;                                                    // persistent scatter workgroups the streams' CU masks leave room for (0: the usual number)
};

inline void overlap_free(OverlapState &ov)
{
    for (int j = 0; j < 2; j++) {
        scatter_free(ov.sc[j]);
        if (ov.side[j]) (void)hipFree(ov.side[j]);
        if (ov.scattered[j]) (void)hipEventDestroy(ov.scattered[j]);
        if (ov.hist_done[j]) (void)hipEventDestroy(ov.hist_done[j]);
    }
    ov = OverlapState();
}

// 0 ok, 1 error, 2 no room, 3 this batch does not fit the overlapped form (several sub-batches): count it with scatter_count
inline int scatter_count_overlapped(OverlapState &ov, const PagedOptions &opt, hipStream_t s_scatter, hipStream_t s_hist, const ScBatch &B, ProfHook &prof)
{
    const int j = ov.next;
    ScatterState &st = ov.sc[j];
    const ScGeom g = scatter_geometry(opt, B.nbytes, B.k, ov.grid);
    if (g.ntiles_all > g.max_tiles) return 3;
    for (int q = 0; q < 2; q++) {
        if ((!ov.scattered[q] && hipEventCreateWithFlags(&ov.scattered[q], hipEventDisableTiming) != hipSuccess) ||
            (!ov.hist_done[q] && hipEventCreateWithFlags(&ov.hist_done[q], hipEventDisableTiming) != hipSuccess)) { partition_error_ref() = "event creation failed"; return 1; }
    }
    // this set's pages are read by the pass of the batch before last: the scatter stream waits for it (and a reallocation drains it)
    if (ov.used[j] && hipStreamWaitEvent(s_scatter, ov.hist_done[j], 0) != hipSuccess) { partition_error_ref() = "stream wait failed"; return 1; }
    // The side list takes one pair per degenerate group that finds its slot of the workgroup's table taken, and one per slot at the end of the
    // kernel.  A group is at most one per wave and window slot: sixteen per wave of 64 chunks and tile -- nbytes / 64 and a little for the tiles'
    // last chunks --, so the list is sized from the batch (a fixed 65536 on top of the drain's pairs overflowed on a few MB of short-period repeats
    // with many distinct units).  The largest batch that comes this far -- one sub-batch, 2 Gi positions -- makes 2^25 pairs: 512 MiB a list.
    const size_t npages = sub_batch(g, 0, 0).npages;
    const size_t side_need = (size_t)g.ntiles_all * (g.tile_pos / 16u + 1u) / 4u + (size_t)g.Gmax * SC_HOT;
    if ((st.cap < npages || st.bkt_cap < (size_t)g.nb) && ov.used[j] && hipEventSynchronize(ov.hist_done[j]) != hipSuccess) return reserve_error(1);
    { const int rc = scatter_reserve(st, s_scatter, npages, (size_t)g.nb); if (rc) return rc; }
    if (ov.side_cap < side_need) {
        const size_t side_new = side_need + side_need / 4;                // (grow-only, with headroom: a reallocation drains both passes)
        for (int q = 0; q < 2; q++) {
            if (ov.side[q]) { if (ov.used[q] && hipEventSynchronize(ov.hist_done[q]) != hipSuccess) return reserve_error(1); (void)hipFree(ov.side[q]); ov.side[q] = nullptr; }
            if (hipMalloc((void **)&ov.side[q], (2 + 2 * side_new) * sizeof(unsigned long long)) != hipSuccess) { (void)hipGetLastError(); ov.side_cap = 0; return reserve_error(2); }
        }
        ov.side_cap = side_new;
    }
    hipLaunchKernelGGL(hot_side_kernel, dim3(1), dim3(1), 0, s_scatter, B.d_ctr, ov.side[j], (unsigned long long)ov.side_cap);
    ScLaunch L;
    if (scatter_stage1(st, opt, s_scatter, g, 0, B, prof, &L)) return 1;
    hipLaunchKernelGGL(hot_side_kernel, dim3(1), dim3(1), 0, s_scatter, B.d_ctr, (unsigned long long *)nullptr, 0ull);      // (whatever runs next on this stream adds directly again)
    if (hipEventRecord(ov.scattered[j], s_scatter) != hipSuccess || hipStreamWaitEvent(s_hist, ov.scattered[j], 0) != hipSuccess) { partition_error_ref() = "stream error"; return 1; }
    if (scatter_stage2(st, s_hist, g, L, B, prof)) return 1;
    hipLaunchKernelGGL(apply_hot_kernel, dim3(8), dim3(256), 0, s_hist, (const unsigned long long *)ov.side[j], B.d_table);
    if (hipGetLastError() != hipSuccess || hipEventRecord(ov.hist_done[j], s_hist) != hipSuccess) { partition_error_ref() = "paged scatter failed to launch"; return 1; }
    ov.used[j] = true;
    ov.last = j;
    ov.next = j ^ 1;
    return 0;
}

// ---------------------------------------------------------------------------------
// host: 13 <= k <= 17, two levels.   id = [ hi : 9 (k = 17: 10) ][ d1 : 2k - 24 (k = 17: 9) ][ d2 : 9 ][ lo : 6 ]
//   level 1  scatter_bases_kernel   residues -> u32 remainders (id without d1), pages tagged d1
//   level 2  scatter_ids_kernel     those pages -> u16 bins (hi | lo), pages tagged d1 << 9 | d2, into an ARENA that
//                                   several batches share
//   flush    one counting sort of the arena's tags, one page_hist_kernel: the sweep over the 4^k vector (8 GiB at
//            k = 15, 128 GiB at k = 17: more than everything else in a batch) is paid once per <= PAGED_PENDING_MAX batches,
//            at kdb_sync / kdb_finish, or when the arena is full -- not once per batch
// ---------------------------------------------------------------------------------
constexpr int PAGED_PENDING_MAX = 64;
// a level-1 ring must take the arrivals of a round (8176 ids x ROUND / 16 / rings, spread evenly by the mid-bit digits) on
// top of an incomplete line:
constexpr int L1_RINGS = 256, L1_C = 64, L1_ROUND = 8;      // k <= 16 (<= 256 digits), u24 elements (64 KiB of LDS): 16 arrivals a round, two flush rounds per tile
// k = 17 (512 digits), u32 elements (64 KiB): 8 arrivals a round on top of < 16 left over, two rounds per tile.  (Four rounds of 4 never
// refuse an element but pay four barrier pairs: level 1 2.46-2.54 ms; two rounds repeat one for ~0.02 % of the rings: 2.09 ms.)
constexpr int L1W_RINGS = 512, L1W_C = 32, L1W_ROUND = 8;
// (128 rings x 128 elements with one round per tile: 2.30 ms as u32, 2.6-2.7 ms as u24 against 2.28 ms for 256 x 64 -- measured, k = 13..15)

struct TwoLevelPaged {
    ScatterState l1;                       // level-1 pages / tags / list (reused by every batch)
    ScatterState arena;                    // level-2 pages of the pending batches
    uint32_t *d_wg_range = nullptr;        // [SC_GRID + 1] of the batch being scattered
    size_t used2 = 0;                      // arena pages the pending batches can have taken at most (their worst cases added up)
    // What they really took is only known on the device: l2_plan_kernel hands every batch the pages behind the previous one's
    // last (d_cursor), not the host's worst case -- round 3 charged a fixed ~0.4 GiB per batch, four times the payload of a
    // 64 MiB host-fed chunk.  The host learns the cursor by asynchronous read-backs (a few probes in flight, polled before
    // every batch) and then only has to assume the worst for the batches behind the last probe that has landed.
    static constexpr int PROBES = 8;
    uint32_t *d_cursor = nullptr;
    uint32_t *h_probe = nullptr;           // pinned [PROBES]
    hipEvent_t ev_probe[PROBES] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t probe_bound[PROBES] = {0};      // used2 (worst cases added up) when the probe was sent
    bool probe_live[PROBES] = {false};
    int probe_next = 0;
    size_t slack = 0;                      // used2 - slack = the host's present bound on the cursor
    int pending = 0;                       // batches in the arena
    int k_pending = 0;
    size_t budget_decided = 0;             // the arena's size where the option leaves it open (PagedOptions::budget_bytes = 0): decided at first use
    size_t free_at_sizing = 0;             // what hipMemGetInfo reported when the budget was decided
    bool table_is_zero = false;            // the engine cleared the vector and nothing has been added since
    bool filled_up = false;                // the last flush came because the arena was full
    bool grow_failed = false;              // a larger arena could not be allocated: no further attempts
    uint64_t reallocs = 0;                 // (re)allocations of the arena so far
    uint64_t full_flushes = 0;             // flushes forced by a full arena since it got its present size
    uint64_t flushes = 0, flushed_batches = 0;     // histogram passes over the arena so far, and the batches they added to the vector
};

inline void twolevel_paged_free(TwoLevelPaged &tp)
{
    scatter_free(tp.l1);
    scatter_free(tp.arena);
    if (tp.d_wg_range) (void)hipFree(tp.d_wg_range);
    if (tp.d_cursor) (void)hipFree(tp.d_cursor);
    if (tp.h_probe) (void)hipHostFree(tp.h_probe);
    for (int i = 0; i < TwoLevelPaged::PROBES; i++) if (tp.ev_probe[i]) (void)hipEventDestroy(tp.ev_probe[i]);
    tp = TwoLevelPaged();
}

// kdb_reset / after a flush: no batch is pending any more (the cursor is cleared when the next cycle begins; so are the tags, unless
// the flush's sort has read them all and so put them back to "no page")
inline void twolevel_paged_drop(TwoLevelPaged &tp, bool sorted = false)
{
    if (!sorted && tp.used2 - tp.slack > tp.arena.tags_dirty) tp.arena.tags_dirty = tp.used2 - tp.slack;
    tp.used2 = 0; tp.slack = 0; tp.pending = 0;
    for (int i = 0; i < TwoLevelPaged::PROBES; i++) tp.probe_live[i] = false;
}

// what the device has told the host about the cursor so far: the newest probe that has landed decides
inline void twolevel_paged_poll(TwoLevelPaged &tp)
{
    for (int i = 0; i < TwoLevelPaged::PROBES; i++) {
        if (!tp.probe_live[i] || hipEventQuery(tp.ev_probe[i]) != hipSuccess) continue;
        tp.probe_live[i] = false;
        // the cursor stood at `actual` when the worst cases added up to probe_bound: every batch since adds at most its worst case to both
        const size_t actual = tp.h_probe[i], bound = tp.probe_bound[i];
        if (bound >= actual && bound - actual > tp.slack) tp.slack = bound - actual;
    }
    (void)hipGetLastError();               // (hipErrorNotReady of a probe still in flight is no error)
}

// what the host works out once per batch for the two levels (as ScGeom for one)
struct L1Geom : TileGeom {
    bool wide /* k = 17: 512 digits, u32 elements */, wide1 /* level 1 in 128-byte pieces */, wide2 /* level 2 likewise */, one_round;
    int d1, nb1, lo_bits, sub_log2;
    uint32_t nb2, G2;                      // level-2 buckets and workgroups
    size_t page_bytes;
};

inline L1Geom twolevel_geometry(const PagedOptions &opt, size_t nbytes, int k)
{
    L1Geom g;
    g.wide = k == 17;                                                   // 16 bin bits instead of 15
    g.d1 = 2 * k - (g.wide ? 16 : 15) - 9;                              // 2, 4, 6, 8 (k = 13..16), 9 (k = 17)
    g.nb1 = 1 << g.d1;
    g.nb2 = 1u << (g.d1 + 9);
    g.lo_bits = opt.lo_bits ? opt.lo_bits : SC_LO_BITS_TWO_LEVEL;
    // k <= 15 (option l1_one_round): 128 rings of 256 three-byte elements instead of 256 of 128 -- a ring then takes a whole tile's arrivals (128 +- 34 on top of < 64
    // left over) and the tile is placed in ONE round: two barriers and one flush per tile instead of four and two; level 1 1.82 -> 1.67 ms at k = 15 (the 64 lanes of a
    // request meet in 128 rings more often than in 256: not the 30 % the instruction count promised).  k = 16 has 256 digits: 256 rings of 256 elements do not fit.
    g.one_round = opt.l1_one_round != 0 && opt.l1_wide != 0 && !g.wide && (1 << g.d1) <= 128;
    g.rings = g.wide ? L1W_RINGS : (g.one_round ? 128 : L1_RINGS);
    // level-1 elements: 24-bit remainders in three bytes (k <= 16), 25-bit ones in four (k = 17)
    g.page_elems = g.wide ? 256u : 512u;
    g.page_bytes = g.wide ? (size_t)ElemFmt<uint32_t>::PAGE_BYTES : (size_t)ElemFmt<u24>::PAGE_BYTES;
    g.sub_log2 = 0;
    while ((g.nb1 << g.sub_log2) < g.rings) g.sub_log2++;
    // level 1 in 128-byte pieces (option l1_wide_lines): one workgroup of 1024 threads per CU, rings of twice the elements, tiles of 1023 chunks
    g.wide1 = opt.l1_wide != 0;
    tile_geometry(g, nbytes, g.wide1 ? (uint32_t)SC1_THREADS - 1u : (uint32_t)SC_TILE_STRIDE, opt.grid > 0 ? (uint32_t)opt.grid : (uint32_t)(g.wide1 ? SC1_GRID : SC_GRID));
    g.wide2 = opt.l2_wide != 0;                                         // level 2 in 128-byte pieces: one workgroup of 1024 threads per CU
    g.G2 = g.wide2 ? (uint32_t)SC1_GRID : (uint32_t)SC_GRID;
    return g;
}

// the histogram pass over everything in the arena
inline int twolevel_paged_flush(TwoLevelPaged &tp, const PagedOptions &opt, hipStream_t stream, unsigned long long *d_table, DevCounters *d_ctr, ProfHook &prof)
{
    if (tp.pending == 0) return 0;
    const L1Geom g = twolevel_geometry(opt, 0, tp.k_pending);
    const int table_is_zero = tp.table_is_zero ? 1 : 0;
    tp.table_is_zero = false;
    twolevel_paged_poll(tp);
    const uint32_t npages = (uint32_t)(tp.used2 - tp.slack);            // (an upper bound on the cursor: tags behind it say "no page")
    // npages = 0: the device's cursor has told the host that the pending batches took no page at all (not one countable window among them: reads of
    // N's in drop mode): nothing to sort, nothing to add -- and a launch with an empty grid is an error (found by tests/fuzz_gpu.py, round 4)
    if (npages != 0) {
        uint32_t slice_pages = (npages + 2047u) / 2048u;
        if (slice_pages < 128u) slice_pages = 128u;
        prof.begin_on(KDB_KERNEL_PAGE_SORT, stream);
        const int src = page_sort(stream, tp.arena, npages, g.nb2, &d_ctr->pages_ids, 32u, slice_pages, 2048u /* (small chunks: few leading digits per LDS window) */, nullptr);
        prof.end();
        if (src) return src;
        prof.begin_on(KDB_KERNEL_PAGE_HIST, stream);
        hist_pass(stream, g.wide, tp.arena, npages, g.nb2, slice_pages, d_table, g.lo_bits, g.lo_bits + g.d1 + 9, table_is_zero, d_ctr);
        prof.end();
    }
    tp.flushes++; tp.flushed_batches += (uint64_t)tp.pending;
    twolevel_paged_drop(tp, tp.arena.tags_dirty == 0);                  // (npages = 0: no tag was written)
    if (hipGetLastError() != hipSuccess) { partition_error_ref() = "histogram pass over the page arena failed to launch"; return 1; }
    return 0;
}

// level-1 scratch for the largest sub-batch, and the small arrays; 0 ok, 1 error, 2 no room
inline int twolevel_ensure_scratch(TwoLevelPaged &tp, hipStream_t stream, const L1Geom &g, int n_expand)
{
    { const int rc = scatter_reserve(tp.l1, stream, sub_batch(g, 0, n_expand).npages, (size_t)g.nb1, g.page_bytes); if (rc) return rc; }
    if (!tp.d_wg_range && hipMalloc((void **)&tp.d_wg_range, (SC_GRID + 1) * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); return reserve_error(2); }
    if (!tp.d_cursor) {
        if (hipMalloc((void **)&tp.d_cursor, sizeof(uint32_t)) != hipSuccess ||
            hipHostMalloc((void **)&tp.h_probe, TwoLevelPaged::PROBES * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return reserve_error(2); }
        for (int i = 0; i < TwoLevelPaged::PROBES; i++)
            if (hipEventCreateWithFlags(&tp.ev_probe[i], hipEventDisableTiming) != hipSuccess) { partition_error_ref() = "event creation failed"; return 1; }
    }
    return bkt_reserve(tp.arena, stream, g.nb2);
}

// a new arena of want_cap pages (nothing is pending); 0 ok, 1 stream error, 2 no room
inline int arena_allocate(TwoLevelPaged &tp, hipStream_t stream, size_t want_cap, size_t need2)
{
    if (hipStreamSynchronize(stream) != hipSuccess) return 1;
    const size_t old_cap = tp.arena.cap;
    page_set_free(tp.arena);
    // what is wanted; failing that what there was (and no further attempts to grow); failing that just this batch
    const size_t tries[3] = {want_cap, old_cap >= need2 ? old_cap : need2, need2};
    for (int attempt = 0; attempt < 3 && !tp.arena.pages; attempt++) {
        if (attempt && tries[attempt] == tries[attempt - 1]) continue;
        if (page_set_alloc(tp.arena, tries[attempt], SC_PAGE_BYTES) == 0 && attempt) tp.grow_failed = true;
    }
    tp.reallocs++;
    tp.full_flushes = 0;
    return tp.arena.pages ? 0 : reserve_error(2);
}

// room in the arena for need2 more pages (acquired before any kernel of the sub-batch runs: "no room" must leave nothing counted):
// flushes what is pending if it must, (re)allocates, and begins a new cycle if nothing is pending.  0 ok, 1 error, 2 no room
inline int arena_room(TwoLevelPaged &tp, const PagedOptions &opt, hipStream_t stream, int k, size_t need2, unsigned long long *d_table, DevCounters *d_ctr, ProfHook &prof)
{
    if (opt.budget_bytes == 0 && tp.budget_decided == 0) {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        // 85 % of what is free now (the vector and level 1's scratch are allocated already): every batch more in the arena
        // makes the sweep of the 4^k vector cheaper per batch (k = 17: 61 ms per flush, 24 batches at 70 % -> 2.5 ms each)
        tp.free_at_sizing = free_b;
        tp.budget_decided = free_b / 100 * 85;
        // (a job that ends in a reduce: RCCL allocates its channel and peer-to-peer buffers at the first collective of each kind, and the
        //  sharded reduce shapes want a chunk of scratch -- the arena, which sizes itself on what is free, must not have taken that room)
        if (opt.reserve_bytes && tp.budget_decided + opt.reserve_bytes > free_b) tp.budget_decided = free_b > opt.reserve_bytes ? free_b - opt.reserve_bytes : 0;
        if (tp.budget_decided > (192ull << 30)) tp.budget_decided = 192ull << 30;
        if (tp.budget_decided < (1ull << 30)) tp.budget_decided = 1ull << 30;
    }
    size_t budget_pages = opt.defer ? (opt.budget_bytes ? opt.budget_bytes : tp.budget_decided) / SC_PAGE_BYTES : 0;
    if (tp.grow_failed && budget_pages > tp.arena.cap) budget_pages = tp.arena.cap;       // (a larger arena could not be had: what there is, is the budget)
    if (budget_pages < need2) budget_pages = need2;
    // worth enlarging: the arena filled up, a quarter more (at least) is within the budget -- and the larger arena pays.
    // Fresh device memory costs ~46 ms per GiB on this runtime (hipMalloc of 128 GiB: 5.9 s, tools/malloc_time.py); a flush
    // forced by a full arena costs one sweep of the vector (16 B per counter at ~5.5 TB/s: 50 ms at k = 17, 3 ms at k = 15),
    // and twice the arena saves every second one.  The arena doubles once the sweeps it would have saved so far add up to
    // the price of the allocation (so a job never spends more than about twice what the best fixed size would have cost
    // it): k = 17 after ~90 forced flushes at 8 batches per flush, k <= 15 in effect never.
    bool may_grow = tp.filled_up && tp.arena.cap + tp.arena.cap / 4 <= budget_pages && opt.grow != 0;
    if (may_grow && opt.grow == 1) {
        const size_t next_cap = 2 * tp.arena.cap < budget_pages ? 2 * tp.arena.cap : budget_pages;
        const double alloc_ms = (double)next_cap * (double)SC_PAGE_BYTES / (double)(1ull << 30) * 46.0;
        const double sweep_ms = (double)(1ull << (2 * k)) * 16.0 / 5.5e9;
        may_grow = (double)tp.full_flushes * sweep_ms * 0.5 >= alloc_ms;
    }
    twolevel_paged_poll(tp);
    if (tp.used2 - tp.slack + need2 > tp.arena.cap || tp.arena.cap == 0 || may_grow) {
        if (tp.pending) { if (twolevel_paged_flush(tp, opt, stream, d_table, d_ctr, prof)) return 1; }
        tp.filled_up = false;
        // The arena grows with the job: room for eight batches like this one at first, twice as much every time it has
        // filled up, until the budget is reached -- a small job (or several processes on one device) never holds tens
        // of GiB it does not use, a long one amortises the sweep of the vector over as many batches as fit.
        size_t want_cap = tp.arena.cap == 0 ? (size_t)opt.first_batches * need2 : 2 * tp.arena.cap;
        if (want_cap > budget_pages) want_cap = budget_pages;
        if (want_cap < need2) want_cap = need2;
        if (tp.arena.cap < need2 || (may_grow && tp.arena.cap < want_cap) || tp.arena.cap == 0) {
            const int rc = arena_allocate(tp, stream, want_cap, need2);
            if (rc) return rc;
        }
    }
    if (tp.pending == 0) {
        // a new cycle: the cursor goes back to the start of the arena, and the tags the last cycle (or a fresh allocation) left behind are cleared
        if (hipMemsetAsync(tp.d_cursor, 0, sizeof(uint32_t), stream) != hipSuccess) { partition_error_ref() = "memset failed"; return 1; }
        if (tags_clean(tp.arena, stream)) return 1;
    }
    return 0;
}

inline BasesPair select_level1(const L1Geom &g, const PagedOptions &opt, int k, int n_expand, int canonical)
{
    const bool compiled15 = !g.wide && k == 15 && !n_expand && canonical && g.lo_bits == SC_LO_BITS_TWO_LEVEL && opt.l1k;
    const bool compiled17 = g.wide && g.wide1 && !n_expand && canonical && g.lo_bits == SC_LO_BITS_TWO_LEVEL && opt.l1k;      // BASELINE config 4's level 1, likewise
    // (k = 14 and k = 16 likewise, canonical drop mode: the kernels of the default path)
    const bool compiled14 = !g.wide && k == 14 && !n_expand && canonical && g.lo_bits == SC_LO_BITS_TWO_LEVEL && opt.l1k;
    const bool compiled16 = !g.wide && k == 16 && !n_expand && canonical && g.lo_bits == SC_LO_BITS_TWO_LEVEL && opt.l1k;
    if (g.one_round) {
        if (compiled15) return bases_pair<uint32_t, u24w, 128, 256, 16, SC1_THREADS, false, true, 15>();
        if (compiled14) return bases_pair<uint32_t, u24w, 128, 256, 16, SC1_THREADS, false, true, 14>();
        return bases_modes<uint32_t, u24w, 128, 256, 16, SC1_THREADS>(n_expand, canonical);
    }
    if (g.wide1) {
        if (compiled16) return bases_pair<uint32_t, u24w, L1_RINGS, 2 * L1_C, L1_ROUND, SC1_THREADS, false, true, 16>();
        if (compiled15) return bases_pair<uint32_t, u24w, L1_RINGS, 2 * L1_C, L1_ROUND, SC1_THREADS, false, true, 15>();
        if (!g.wide) return bases_modes<uint32_t, u24w, L1_RINGS, 2 * L1_C, L1_ROUND, SC1_THREADS>(n_expand, canonical);
        if (compiled17) return bases_pair<uint64_t, u32w, L1W_RINGS, 2 * L1W_C, L1W_ROUND, SC1_THREADS, false, true, 17>();
        return bases_modes<uint64_t, u32w, L1W_RINGS, 2 * L1W_C, L1W_ROUND, SC1_THREADS>(n_expand, canonical);
    }
    // BASELINE config 3's kernel with its shifts and masks compiled in (as the k = 12 headline's)
    if (compiled15) return bases_pair<uint32_t, u24, L1_RINGS, L1_C, L1_ROUND, SC_THREADS, false, true, 15>();
    if (!g.wide) return bases_modes<uint32_t, u24, L1_RINGS, L1_C, L1_ROUND, SC_THREADS>(n_expand, canonical);
    return bases_modes<uint64_t, uint32_t, L1W_RINGS, L1W_C, L1W_ROUND, SC_THREADS>(n_expand, canonical);
}

// level 2's kernel: 1024 threads (SC1_THREADS) where it writes 128-byte pieces, else 512 (SC_THREADS)
inline IdsKernel select_level2(const L1Geom &g, const PagedOptions &opt)
{
    const bool fixed2 = g.lo_bits == SC_LO_BITS_TWO_LEVEL && opt.l1k;   // (shifts and masks compiled in)
    if (g.wide2) {
        if (g.wide) return fixed2 ? scatter_ids_kernel<uint32_t, u16w, 512, 128, true, SC1_THREADS> : scatter_ids_kernel<uint32_t, u16w, 512, 128, false, SC1_THREADS>;
        return fixed2 ? scatter_ids_kernel<u24, u16w, 512, 128, true, SC1_THREADS> : scatter_ids_kernel<u24, u16w, 512, 128, false, SC1_THREADS>;
    }
    if (g.wide) return scatter_ids_kernel<uint32_t, uint16_t, 512, 64, false, SC_THREADS>;
    return fixed2 ? scatter_ids_kernel<u24, uint16_t, 512, 64, true, SC_THREADS> : scatter_ids_kernel<u24, uint16_t, 512, 64, false, SC_THREADS>;
}

// level 1 of sub-batch L: scatter, page sort, level 2's plan; the arena is charged need2 pages and a probe of the cursor is sent
inline int twolevel_level1(TwoLevelPaged &tp, const PagedOptions &opt, hipStream_t stream, const L1Geom &g, const ScLaunch &L, uint64_t t0, size_t need2, const ScBatch &B,
                           ProfHook &prof)
{
    if (launch_bases(select_level1(g, opt, B.k, B.n_expand, B.canonical), stream, prof, tp.l1, L, opt.contig_pages, B, t0, g.lo_bits + 9, g.d1, g.sub_log2))
        return 1;
    prof.begin_on(KDB_KERNEL_PAGE_SORT, stream);
    if (page_sort(stream, tp.l1, L.npages, (uint32_t)g.nb1, &B.d_ctr->pages_bases, g.wide ? 16u : 32u, 1u << 20, 256u, B.d_ctr)) { prof.end(); return 1; }
    hipLaunchKernelGGL(l2_plan_kernel, dim3(1), dim3(1024), 0, stream, (const uint32_t *)bkt_arrays(tp.l1, (size_t)g.nb1).page_base, (uint32_t)g.nb1, g.G2, 512u, g.page_elems, tp.d_wg_range, tp.d_cursor,
                       (uint32_t)tp.arena.cap, B.d_ctr);
    prof.end();
    tp.used2 += need2;
    // tell the host where the cursor stands now (a probe slot that is still in flight is left alone: the bound stays valid without it)
    const int pi = tp.probe_next;
    if (!tp.probe_live[pi] && hipMemcpyAsync(&tp.h_probe[pi], tp.d_cursor, sizeof(uint32_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
        hipEventRecord(tp.ev_probe[pi], stream) == hipSuccess) {
        tp.probe_live[pi] = true; tp.probe_bound[pi] = tp.used2;
        tp.probe_next = (pi + 1) % TwoLevelPaged::PROBES;
    }
    return 0;
}

// level 2 of the sub-batch that level 1 has just sorted, into the pages l2_plan_kernel gave it; then the histogram pass if it is due
inline int twolevel_level2(TwoLevelPaged &tp, const PagedOptions &opt, hipStream_t stream, const L1Geom &g, size_t need2, const ScBatch &B, ProfHook &prof)
{
    ScOut out2;
    out2.pages = tp.arena.pages; out2.tag = tp.arena.tag; out2.wg_pages = 0; out2.wg_range = tp.d_wg_range; out2.contig = 0; out2.wg_base = 0; out2.grid = 0; out2.extra_elems = 0;
    const IdsKernel fn = select_level2(g, opt);
    prof.begin_on(KDB_KERNEL_SCATTER_L2, stream);
    hipLaunchKernelGGL(fn, dim3(g.G2), dim3(g.wide2 ? SC1_THREADS : SC_THREADS), 0, stream, (const uint8_t *)tp.l1.pages, (const PageEntry *)tp.l1.list,
                       (const uint32_t *)bkt_arrays(tp.l1, (size_t)g.nb1).page_base, (uint32_t)g.nb1, g.lo_bits, 9, out2, B.d_ctr);
    prof.end();
    tp.pending++;
    tp.k_pending = B.k;
    if (hipGetLastError() != hipSuccess) { partition_error_ref() = "two-level paged scatter failed to launch"; return 1; }
    // flush now if told not to defer, after PAGED_PENDING_MAX batches, or when another batch like this one would not fit the arena
    const bool full = tp.used2 - tp.slack + need2 > tp.arena.cap;
    if (opt.defer && full) { tp.filled_up = true; tp.full_flushes++; }      // (the next batch finds the arena empty and may enlarge it)
    if (!opt.defer || tp.pending >= PAGED_PENDING_MAX || full) return twolevel_paged_flush(tp, opt, stream, B.d_table, B.d_ctr, prof);
    return 0;
}

// returns 0 ok, 1 error (partition_error()), 2 no room for the scratch (nothing of the batch was counted)
inline int twolevel_paged_count(TwoLevelPaged &tp, const PagedOptions &opt, hipStream_t stream, const ScBatch &B, size_t max_windows /* nbytes - records x (k - 1) */,
                                ProfHook &prof)
{
    const L1Geom g = twolevel_geometry(opt, B.nbytes, B.k);
    if (tp.pending && tp.k_pending != B.k) { if (twolevel_paged_flush(tp, opt, stream, B.d_table, B.d_ctr, prof)) return 1; }
    { const int rc = twolevel_ensure_scratch(tp, stream, g, B.n_expand); if (rc) return rc; }
    for (uint64_t t0 = 0; t0 < g.ntiles_all; t0 += g.max_tiles) {
        const ScLaunch L = sub_batch(g, t0, B.n_expand);
        // what level 2 can need at most (l2_plan_kernel hands out exactly what it does need, within this)
        // (a page per 512 of the elements level 1 can emit -- at most one per position, N expansions go straight to the vector --
        //  plus level 1's partial pages rounded up, plus a partial page per ring and digit span of every level-2 workgroup)
        //  A batch of records that are all at least k long has nbytes - records x (k - 1) windows; one that is not fails at the
        //  sync, and until then a scatter kernel that runs out of its page sequence stops writing (internal_err), never out of bounds.
        // (N-expansion mode: plus the fills of N-windows that level 1 may send through its rings)
        const size_t pos = (size_t)L.nt * g.tile_pos, elems = (pos < max_windows ? pos : max_windows) + (size_t)L.G * L.extra_elems;
        const size_t need2 = (elems + 511) / 512 + (size_t)L.G * (size_t)g.rings + 2 * (size_t)g.G2 + 512 * ((size_t)g.nb1 + g.G2) + 16;
        const int rc = arena_room(tp, opt, stream, B.k, need2, B.d_table, B.d_ctr, prof);
        if (rc) return rc == 2 && t0 != 0 ? 1 : rc;                   // (no room behind the first sub-batch: part of the batch is counted already)
        if (twolevel_level1(tp, opt, stream, g, L, t0, need2, B, prof)) return 1;
        if (twolevel_level2(tp, opt, stream, g, need2, B, prof)) return 1;
    }
    return 0;
}

#ifdef KDB_SC_PROF
// What the scatter kernels of a -DKDB_SC_PROF build have stamped since the last report (kdb_sync calls it with the device idle): their
// wave-cycles by phase, and when the workgroups of each kernel's last launch ended (KDB_SC_WG_DUMP=file: every workgroup's); to stderr.
inline void sc_prof_report()
{
    unsigned long long h[32];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_sc_prof), sizeof h) != hipSuccess || !(h[8] || h[24])) return;
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
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sc_prof), h, sizeof h);
    // the last launch of each kernel: when its workgroups ended, relative to the launch's span
    static unsigned long long wg[2][2][1024];
    if (hipMemcpyFromSymbol(wg, HIP_SYMBOL(g_sc_wg), sizeof wg) != hipSuccess) return;
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
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sc_wg), wg, sizeof wg);
}
#endif

}  // namespace kdb
