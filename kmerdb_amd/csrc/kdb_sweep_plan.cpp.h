// kdb_sweep_plan.cpp.h -- the host-only plans of the analysis calls (plain C++, no HIP: tests/c/sweep_plan_check.cpp compiles it alone, runs
// it under the sanitizers and prints the plans for tests/sweep_cases.py to be compared with): which block pairs become which launch rows,
// in which order and under which kernel instantiation (kdb_gram, kdb_pairstats, kdb_pairfloat), the grid of a sweep, the one check of record
// offsets (check_offsets) and the one split of records into pieces (RecordLayout, record_layout) that kdb_score_reads, kdb_record_tables
// (tests/c/tables_plan_check.cpp) and kdb_minimizers (tests/c/minimizers_plan_check.cpp) share -- each adds how many windows a record has and
// what else it asks of its records --, and the window, the stages and the LDS of a task of kdb_align_banded (tests/c/alignment_plan_check.cpp) and the
// direction scratch and the chunks of kdb_align_traceback (tests/c/traceback_plan_check.cpp).
// The block size, HALF, the chunk sizes, the piece size and the stage are arguments: the kernel headers have them.
// A row type is the kernel header's (kdbgram::Row, kdbpair::Row, kdbpair::FloatRow) or any struct of as many uint8_t fields.
#pragma once
#include <cstdint>

#include <algorithm>
#include <vector>

namespace kdbplan {

// rows row0 .. row0 + nrows are one launch, of the instantiation <na, nb, diag>
struct Group { uint32_t row0, nrows; int na, nb; bool diag; };

template <class Row>
struct Plan {
    std::vector<Row> rows;
    std::vector<Group> groups;
    // a row joins the last group if that has its instantiation, else it opens one
    void push(const Row &row, int na, int nb, bool diag)
    {
        if (groups.empty() || groups.back().na != na || groups.back().nb != nb || groups.back().diag != diag)
            groups.push_back(Group{(uint32_t)rows.size(), 0, na, nb, diag});
        groups.back().nrows++;
        rows.push_back(row);
    }
};

// kdb_gram: rows = pairs of blocks of B vectors (bi <= bj); the last block may hold fewer than B.  The full diagonal blocks, the pairs of
// full blocks (bi-major), the short last block's diagonal, every full block against the short one.
template <class Row>
Plan<Row> gram_plan(int n, int B)
{
    const int nblk = (n + B - 1) / B, last = n - (nblk - 1) * B, nfull = last == B ? nblk : nblk - 1;
    Plan<Row> p;
    auto push = [&](int bi, int bj, int na, int nb) { p.push(Row{(uint8_t)bi, (uint8_t)bj}, na, nb, bi == bj); };
    for (int b = 0; b < nfull; b++) push(b, b, B, B);
    for (int bi = 0; bi < nfull; bi++) for (int bj = bi + 1; bj < nfull; bj++) push(bi, bj, B, B);
    if (nfull < nblk) {
        push(nfull, nfull, last, last);
        for (int bi = 0; bi < nfull; bi++) push(bi, nfull, B, last);
    }
    return p;
}

// kdb_pairstats: rows = vectors a0 .. a0 + na against b0 .. b0 + nb.  The diagonal blocks (the last may hold fewer than B vectors), then
// every earlier block against the later blocks' vectors, HALF at a time: the rows of HALF vectors first, then the rows of a single one
// (two groups at most).
template <class Row>
Plan<Row> pair_plan(int n, int B, int HALF)
{
    const int nblk = (n + B - 1) / B;
    auto block_size = [&](int b) { return std::min(B, n - b * B); };
    Plan<Row> p;
    auto push = [&](int a0, int na, int b0, int nb) { p.push(Row{(uint8_t)a0, (uint8_t)na, (uint8_t)b0, (uint8_t)nb}, na, nb, a0 == b0); };
    for (int b = 0; b < nblk; b++) push(b * B, block_size(b), b * B, block_size(b));
    for (int pass = 0; pass < 2; pass++)
        for (int bj = 1; bj < nblk; bj++)
            for (int h = 0; h < block_size(bj); h += HALF) {
                const int nb = std::min(HALF, block_size(bj) - h);
                if ((nb == HALF) != (pass == 0)) continue;
                for (int bi = 0; bi < bj; bi++) push(bi * B, B, bj * B + h, nb);
            }
    return p;
}

// kdb_pairfloat: one pair i < j per row
template <class Row>
std::vector<Row> float_rows(int n)
{
    std::vector<Row> rows;
    for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++) rows.push_back(Row{(uint8_t)i, (uint8_t)j});
    return rows;
}

// The grid of a sweep whose waves step through chunks of chunk_bins bins, wg_chunks waves to a workgroup: gx workgroups per row, each with
// a partial of its own.  tail: a tail kernel takes the bins behind the last whole chunk and writes one more partial (nparts = gx + 1);
// without one the last, partial chunk is the body's.
struct Grid { uint32_t nchunks, gx, nparts; };

inline Grid sweep_grid(uint64_t nbins, uint32_t chunk_bins, uint32_t wg_chunks, uint32_t cap, bool tail = true)
{
    const uint32_t nchunks = (uint32_t)((nbins + (tail ? 0 : chunk_bins - 1)) / chunk_bins);
    const uint32_t gx = std::max(1u, std::min((nchunks + wg_chunks - 1) / wg_chunks, cap));
    return Grid{nchunks, gx, gx + 1};
}

// the most workgroups per row of a sweep with nrows rows: from many_rows rows on the rows fill the device and the smaller cap does
inline uint32_t rows_cap(uint32_t nrows, uint32_t many_rows, uint32_t cap, uint32_t cap_many_rows) { return nrows < many_rows ? cap : cap_many_rows; }

// The per-record calls (kdb_score_reads, kdb_record_tables, kdb_minimizers) take nbytes residues and the nreads + 1 offsets of their records,
// nreads >= 1, and share one layout; kdb_align_banded takes two such buffers.
enum LayoutError { LAYOUT_OK = 0, LAYOUT_ENDS /* must start at 0 and end at nbytes */, LAYOUT_RISE /* must rise from 0 to nbytes */,
                   LAYOUT_ENTRIES /* kdb_record_tables: more table entries than the call allows */,
                   LAYOUT_TASK, LAYOUT_STRAND, LAYOUT_QUERY /* kdb_align_banded: a task's record index, its strand, its query's length */ };

// offs: n + 1 offsets into nbytes residues; where both fail it is LAYOUT_ENDS.  each(r, len) is given the records in order, in the same
// pass, as far as their offsets rise.
template <class Each>
LayoutError check_offsets(const uint64_t *offs, size_t n, uint64_t nbytes, Each each)
{
    if (offs[0] != 0 || offs[n] != nbytes) return LAYOUT_ENDS;
    for (size_t r = 0; r < n; r++) {
        if (offs[r + 1] < offs[r] || offs[r + 1] > nbytes) return LAYOUT_RISE;
        each(r, offs[r + 1] - offs[r]);
    }
    return LAYOUT_OK;
}

inline LayoutError check_offsets(const uint64_t *offs, size_t n, uint64_t nbytes) { return check_offsets(offs, n, nbytes, [](size_t, uint64_t) {}); }

// Record r is pieces rec_piece0[r] .. rec_piece0[r + 1], of at most `piece` windows each and at least one (a record without a window has
// an empty one); piece_rec[p] = the record of piece p, left empty when every record is one piece.  A refused layout is an empty one.
struct RecordLayout {
    std::vector<uint32_t> rec_piece0, piece_rec;
    uint64_t npieces = 0;
};

// The layout (a RecordLayout, or a call's own with more members) of the records that check_offsets() passes.  windows(r, len): how many
// windows record r, of len residues, has -- all a call has of its own here.  It is asked once per record, in order, so it may note in
// `lay` what else the call wants to know of its records.
template <class Layout, class Windows>
LayoutError record_layout(const uint64_t *offs, size_t nreads, uint64_t nbytes, uint32_t piece, Windows windows, Layout &lay)
{
    lay = Layout();
    lay.rec_piece0.resize(nreads + 1);
    const LayoutError bad = check_offsets(offs, nreads, nbytes, [&](size_t r, uint64_t len) {
        lay.rec_piece0[r] = (uint32_t)lay.npieces;
        lay.npieces += std::max<uint64_t>(1, (windows(r, len) + piece - 1) / piece);                       // (< 2^31: 2^30 records and 2^30 windows at most)
    });
    if (bad) {
        lay = Layout();
        return bad;
    }
    lay.rec_piece0[nreads] = (uint32_t)lay.npieces;
    if (lay.npieces != nreads) {
        lay.piece_rec.resize(lay.npieces);
        for (size_t r = 0; r < nreads; r++)
            for (uint32_t p = lay.rec_piece0[r]; p < lay.rec_piece0[r + 1]; p++) lay.piece_rec[p] = (uint32_t)r;
    }
    return LAYOUT_OK;
}

// kdb_score_reads: a record of len residues has the windows 0 .. len - k.  One shorter than k counts as short unless it is the first and
// `continues` an earlier call's; where there are short records piece_rec is left empty: the caller refuses them.
struct ScoreLayout : RecordLayout { uint64_t nshort = 0; };

inline LayoutError score_layout(const uint64_t *offs, size_t nreads, uint64_t nbytes, int k, uint32_t piece, bool continues, ScoreLayout &lay)
{
    auto windows = [&](size_t r, uint64_t len) {
        if (len < (uint64_t)k && !(r == 0 && continues)) lay.nshort++;
        return len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0;
    };
    const LayoutError bad = record_layout(offs, nreads, nbytes, piece, windows, lay);
    if (lay.nshort) lay.piece_rec.clear();
    return bad;
}

// kdb_record_tables: the windows of a record of len residues start at phase + i stride, for every i with phase + i stride + k <= len
// (constexpr: the kernel counts them with the same expression)
constexpr uint64_t tables_windows(uint64_t len, int k, int stride, uint64_t phase)
{
    return len >= (uint64_t)k + phase ? (len - (uint64_t)k - phase) / (uint64_t)stride + 1 : 0;
}

// Piece p of record r holds the windows (p - rec_piece0[r]) piece .. of the record's tables_windows(), `phase` for record 0 and 0 for the
// others.  multi: the records of more than one piece, in order -- their rows are added to by several waves and are zeroed first; every
// other row is stored whole by its only wave.  LAYOUT_ENTRIES: nreads 4^k is above max_entries.
struct TablesLayout : RecordLayout {
    std::vector<uint32_t> multi;
    // the windows [first, first + count) of piece p of record r, which has nwin of them
    static void piece_windows(uint64_t nwin, uint32_t p_in_rec, uint32_t piece, uint64_t &first, uint32_t &count)
    {
        first = (uint64_t)p_in_rec * piece;
        count = (uint32_t)std::min<uint64_t>(piece, nwin > first ? nwin - first : 0);
    }
};

inline LayoutError tables_layout(const uint64_t *offs, size_t nreads, uint64_t nbytes, int k, int stride, uint64_t phase, uint32_t piece, uint64_t max_entries,
                                 TablesLayout &lay)
{
    lay = TablesLayout();
    if ((uint64_t)nreads > (max_entries >> (2 * k))) {                            // refused, but what its offsets are refused for comes first
        const LayoutError bad = check_offsets(offs, nreads, nbytes);
        return bad ? bad : LAYOUT_ENTRIES;
    }
    auto windows = [&](size_t r, uint64_t len) {
        const uint64_t nwin = tables_windows(len, k, stride, r == 0 ? phase : 0);
        if (nwin > piece) lay.multi.push_back((uint32_t)r);
        return nwin;
    };
    return record_layout(offs, nreads, nbytes, piece, windows, lay);
}

// kdb_minimizers: a record of len residues has the start positions 0 .. len - k (constexpr: the kernels count them with the same expression)
constexpr uint64_t minimizer_positions(uint64_t len, int k) { return len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0; }

// Piece p_in_rec of a record of nwin start positions OWNS the positions [first, first + count) -- it alone decides whether they are
// selected -- and for that READS the keys of the positions [lo, hi): its own and up to w - 1 on either side, cut at the record's ends.
// The residues behind those keys are [lo, hi + k - 1) of the record, all inside it.
struct MinimizerPiece { uint64_t first, lo, hi; uint32_t count; };

constexpr MinimizerPiece minimizer_piece(uint64_t nwin, uint32_t p_in_rec, uint32_t piece, uint32_t w)
{
    const uint64_t first = (uint64_t)p_in_rec * piece;
    const uint64_t left = nwin > first ? nwin - first : 0;
    const uint32_t count = (uint32_t)(left < (uint64_t)piece ? left : (uint64_t)piece);
    const uint64_t halo = (uint64_t)w - 1;
    const uint64_t lo = count == 0 ? first : (first > halo ? first - halo : 0);
    const uint64_t hi = count == 0 ? first : (first + count + halo < nwin ? first + count + halo : nwin);
    return MinimizerPiece{first, lo, hi, count};
}

// The windows of the layout are the start positions.  max_keys: the most keys any piece reads; lds_wave: the bytes of LDS a wave then
// needs, a multiple of 8 -- max_keys keys of 8 bytes, then the residues behind them, read as aligned 4-byte words (up to 3 bytes before
// the first and after the last).
struct MinimizersLayout : RecordLayout { uint32_t max_keys = 0, lds_wave = 0; };

inline LayoutError minimizers_layout(const uint64_t *offs, size_t nreads, uint64_t nbytes, int k, uint32_t w, uint32_t piece, MinimizersLayout &lay)
{
    auto windows = [&](size_t, uint64_t len) {
        const uint64_t nwin = minimizer_positions(len, k);
        for (uint64_t p = 0; p * piece < nwin; p++) {
            const MinimizerPiece pc = minimizer_piece(nwin, (uint32_t)p, piece, w);
            lay.max_keys = std::max(lay.max_keys, (uint32_t)(pc.hi - pc.lo));
        }
        return nwin;
    };
    const LayoutError bad = record_layout(offs, nreads, nbytes, piece, windows, lay);
    if (!bad) lay.lds_wave = lay.max_keys * 8u + ((lay.max_keys + (uint32_t)k + 6u + 7u) & ~7u);
    return bad;
}

// kdb_align_banded: a task aligns an oriented query of m residues to a reference record of n around the diagonal d, j - i = d, inside
// |(j - i) - d| <= band.  With jb = d - band cell (i, j) lies on the band's diagonal c = j - i - jb, 0 <= c <= 2 band.
//   [r_lo, r_hi): the reference residues the band can reach, [d - band, d + m - 1 + band] cut to [0, n)
//   [i_lo, i_hi): the query rows that hold a cell both in the band and in the record; every other row is all zero
// A task whose band misses the record, or with m = 0 or n = 0, is EMPTY: all six are 0.  Otherwise jb fits 32 bits: -m - 2 band < jb < n.
// (constexpr: the kernel asks for the same window.)
struct AlignWindow {
    uint32_t r_lo, r_hi, i_lo, i_hi;
    int32_t jb;
    constexpr bool empty() const { return i_lo >= i_hi; }
};

constexpr AlignWindow align_window(uint64_t m, uint64_t n, int64_t d, uint32_t band)
{
    const int64_t far = (int64_t)1 << 32;                                         // (m <= 2^20, n <= 2^30: a diagonal out there meets nothing)
    if (m == 0 || n == 0 || d >= far || d <= -far) return AlignWindow{0, 0, 0, 0, 0};
    const int64_t jb = d - (int64_t)band, b2 = 2 * (int64_t)band;
    const int64_t i_lo = -jb - b2 > 0 ? -jb - b2 : 0;
    const int64_t i_hi = (int64_t)n - jb < (int64_t)m ? (int64_t)n - jb : (int64_t)m;
    if (i_lo >= i_hi) return AlignWindow{0, 0, 0, 0, 0};
    const int64_t r_lo = jb > 0 ? jb : 0;
    const int64_t r_hi = jb + (int64_t)m + b2 < (int64_t)n ? jb + (int64_t)m + b2 : (int64_t)n;
    return AlignWindow{(uint32_t)r_lo, (uint32_t)r_hi, (uint32_t)i_lo, (uint32_t)i_hi, (int32_t)jb};
}

// The wave sweeps anti-diagonals: in step T lane l works on row T - l, so the rows [i_lo, i_hi) take the steps [t_lo, t_hi), t_lo a
// multiple of ALIGN_GROUP (the rows a lane takes from one pair of LDS reads), in stages of `stage` steps.  A stage that begins at step ts
// holds in LDS the oriented query rows [ts - ALIGN_LANES, ts + stage) and the reference residues [ts - ALIGN_LANES + jb, + stage +
// ALIGN_R_EXTRA) -- the lanes' rows and, ALIGN_LANES - 1 rows back and 2 ALIGN_LANES - 1 diagonals on, what the last group reads -- whatever
// the band is; a row or residue outside the record is staged as a code that matches nothing.
constexpr uint32_t ALIGN_LANES = 64, ALIGN_GROUP = 4, ALIGN_R_EXTRA = 2 * ALIGN_LANES + 8;
constexpr uint32_t align_t_lo(const AlignWindow &w) { return w.i_lo & ~(ALIGN_GROUP - 1); }
constexpr uint32_t align_t_hi(const AlignWindow &w, uint32_t band) { return w.i_hi + band; }
constexpr uint32_t align_stages(const AlignWindow &w, uint32_t band, uint32_t stage)
{
    return w.empty() ? 0 : (align_t_hi(w, band) - align_t_lo(w) + stage - 1) / stage;
}
constexpr uint32_t align_lds_q(uint32_t stage) { return stage + ALIGN_LANES + 8; }    // (+ 8: a lane reads the two aligned words around its 4 rows)
constexpr uint32_t align_lds_r(uint32_t stage) { return stage + ALIGN_R_EXTRA; }
constexpr uint32_t align_lds_wave(uint32_t stage) { return align_lds_q(stage) + align_lds_r(stage); }     // a multiple of 8 where stage is

// kdb_align_traceback: the forward pass leaves 4 bits per cell, and a lane's two diagonals over the ALIGN_GROUP rows of a group are one
// dword: every group of steps of [t_lo, t_hi) is ALIGN_LANES dwords, all 64 lanes' (the lanes beyond the band store theirs too: this is the
// single place that says so).  Cell (i, c) is nibble 2 ((T - t_lo) % ALIGN_GROUP) + (c & 1) of dword align_trace_dword(..), T = i + c / 2.
constexpr uint64_t ALIGN_TRACE_GROUP_BYTES = 4ull * ALIGN_LANES;
constexpr uint32_t align_trace_groups(const AlignWindow &w, uint32_t band)
{
    return w.empty() ? 0 : (align_t_hi(w, band) - align_t_lo(w) + ALIGN_GROUP - 1) / ALIGN_GROUP;
}
constexpr uint64_t align_trace_bytes(const AlignWindow &w, uint32_t band) { return (uint64_t)align_trace_groups(w, band) * ALIGN_TRACE_GROUP_BYTES; }
constexpr uint64_t align_trace_dword(uint32_t group, uint32_t lane) { return (uint64_t)group * ALIGN_LANES + lane; }     // (inside the task's bytes)

// The call works through its tasks in chunks of consecutive tasks: a chunk is the longest run of tasks whose bytes fit `limit`, and holds
// at least one task.  first: nchunks + 1 entries, chunk k is the tasks [first[k], first[k + 1]); offs[t]: where task t's bytes begin in its
// chunk's scratch; largest: the bytes of the largest chunk.
struct AlignTraceChunks {
    std::vector<uint64_t> first, offs;
    uint64_t largest = 0, bytes = 0;
};

inline void align_trace_chunks(const uint64_t *task_bytes, size_t ntasks, uint64_t limit, AlignTraceChunks &ch)
{
    ch = AlignTraceChunks();
    ch.offs.resize(ntasks);
    ch.first.push_back(0);
    uint64_t used = 0;
    for (size_t t = 0; t < ntasks; t++) {
        if (t > ch.first.back() && (used > limit || task_bytes[t] > limit - used)) {     // (a task above the limit is a chunk of its own)
            ch.first.push_back(t);
            used = 0;
        }
        ch.offs[t] = used;
        used += task_bytes[t];
        ch.largest = std::max(ch.largest, used);
        ch.bytes += task_bytes[t];
    }
    if (ntasks) ch.first.push_back(ntasks);
}

// The batch: every offset array must start at 0, end at its buffer's size and rise; every task must name a query and a reference record
// (LAYOUT_TASK, bad = the task) and a strand 0 or 1 (LAYOUT_STRAND), and its query holds at most max_query residues (LAYOUT_QUERY).
// grid: workgroups of `waves` waves, a wave per task, at most grid_max of them (the waves then stride through the tasks).  cells: the sum
// of m (2 band + 1) over the tasks, the figure the benchmark divides by.
struct AlignLayout {
    uint32_t grid = 0;
    uint64_t cells = 0, nonempty = 0, bad = 0;
};

inline LayoutError align_layout(const uint64_t *q_offs, size_t nq, uint64_t q_nbytes, const uint64_t *r_offs, size_t nr, uint64_t r_nbytes, const uint32_t *task_q,
                                const uint32_t *task_r, const int64_t *task_diag, const uint8_t *task_strand, size_t ntasks, uint32_t band, uint64_t max_query,
                                uint32_t waves, uint32_t grid_max, AlignLayout &lay)
{
    lay = AlignLayout();
    const LayoutError bad_q = check_offsets(q_offs, nq, q_nbytes), bad_r = check_offsets(r_offs, nr, r_nbytes);
    if (bad_q || bad_r) return bad_q == LAYOUT_ENDS || bad_r == LAYOUT_ENDS ? LAYOUT_ENDS : LAYOUT_RISE;      // (the ends of both buffers come first)
    uint64_t cells = 0, nonempty = 0;
    for (size_t t = 0; t < ntasks; t++) {
        lay.bad = t;
        if (task_q[t] >= nq || task_r[t] >= nr) return LAYOUT_TASK;
        if (task_strand[t] > 1) return LAYOUT_STRAND;
        const uint64_t m = q_offs[task_q[t] + 1] - q_offs[task_q[t]], n = r_offs[task_r[t] + 1] - r_offs[task_r[t]];
        if (m > max_query) return LAYOUT_QUERY;
        cells += m * (2 * (uint64_t)band + 1);
        nonempty += align_window(m, n, task_diag[t], band).empty() ? 0 : 1;
    }
    lay.bad = 0;
    lay.cells = cells;
    lay.nonempty = nonempty;
    lay.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((ntasks + waves - 1) / waves, grid_max));
    return LAYOUT_OK;
}

}  // namespace kdbplan
