// kdb_engine_options.hip.h -- the engine's plain integer options: the table (one row each), kdb_set_option / kdb_get_option (the odd ones
// are code in those two functions) and the KDB_ENGINE_OPTS environment list that kdb_create applies.  Included by kdb_engine.hip behind
// struct kdb_engine and the helpers an option's "before" action calls (flush_pending_paged, overlap_streams).
#pragma once

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
    {"accum_bytes", KDB_OPT(feed.accum_bytes), false, -1, INT64_MAX, OPT_NO_STAGING, " (-1 auto, 0 off, else bytes)"},
    {"stage_bytes", KDB_OPT(feed.stage_bytes), false, 4096, INT64_MAX, OPT_NO_STAGING, " (>=4096, multiple of 16)", 16},
    {"stage_reads", KDB_OPT(feed.stage_reads), false, 1, INT64_MAX, OPT_NO_STAGING},
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

// KDB_ENGINE_OPTS="name=value,name=value": tuning options for every engine of the process (experiments and the test suite under an
// option: tools/experiments/); an unknown name or a refused value fails the creation -- loudly, like kdb_set_option itself
int engine_env_options(kdb_engine *e)
{
    const char *opts = getenv("KDB_ENGINE_OPTS");
    if (!opts) return KDB_OK;
    const std::string all(opts);
    for (size_t at = 0; at < all.size();) {
        size_t end = all.find(',', at);
        if (end == std::string::npos) end = all.size();
        const std::string kv = all.substr(at, end - at);
        at = end + 1;
        if (kv.empty()) continue;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) return fail(KDB_ERR_ARG, "KDB_ENGINE_OPTS: '%s' is not name=value", kv.c_str());
        const int rc = kdb_set_option(e, kv.substr(0, eq).c_str(), (int64_t)strtoll(kv.c_str() + eq + 1, nullptr, 0));
        if (rc != KDB_OK) return rc;
    }
    return KDB_OK;
}
}  // namespace

extern "C" {

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
    if (row->before == OPT_NO_STAGING && e->feed.staging_ready) return fail(KDB_ERR_STATE, "staging already allocated");
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
                HIP_TRY(hipMemcpy(&v, (const char *)e->d_ctr.p + d.off, sizeof v, hipMemcpyDeviceToHost));
                *value = (int64_t)v;
                return KDB_OK;
            }
    }
    return fail(KDB_ERR_ARG, "unknown option '%s'", name);
}

}  // extern "C"
