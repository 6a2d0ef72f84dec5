// The host plans of the analysis calls (kmerdb_amd/csrc/kdb_sweep_plan.cpp.h) alone, for AddressSanitizer + UBSan on the CPU.  It runs the
// commands of its command line, checks each plan's own invariants and prints the plan as text, for tests/test_sweep_plan_host.py to compare
// with tests/sweep_cases.py:
//     rows B HALF n                        kdb_gram's, kdb_pairstats' and kdb_pairfloat's rows of n vectors, each with its group's instantiation
//     grid nbins chunk wg_chunks cap tail  the grid triple of a sweep
//     cap nrows many cap cap_many          the cap a sweep of nrows rows takes
//     score k piece continues nbytes o,..  the piece layout of records with the offsets o,.. (or its refusal)
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o sweep_plan_check tests/c/sweep_plan_check.cpp && ./sweep_plan_check rows 4 2 5
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kmerdb_amd/csrc/kdb_sweep_plan.cpp.h"

static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); bad++; } } while (0)

// the byte layouts the kernels read
struct GramRow { uint8_t bi, bj; };
struct PairRow { uint8_t a0, na, b0, nb; };
struct FloatRow { uint8_t i, j; };

// the groups partition the rows, in order, and none is empty
static void check_groups(const std::vector<kdbplan::Group> &groups, size_t nrows)
{
    uint32_t at = 0;
    for (const kdbplan::Group &g : groups) {
        CHECK(g.row0 == at && g.nrows > 0);
        at += g.nrows;
    }
    CHECK(at == nrows);
}

// what the launch switches have: <m, m, true> for m = 1 .. B, and <B, nb, false> for the nb of `off`
static void check_inst(const kdbplan::Group &g, int B, const std::vector<int> &off)
{
    if (g.diag) CHECK(g.na == g.nb && g.na >= 1 && g.na <= B);
    else CHECK(g.na == B && std::find(off.begin(), off.end(), g.nb) != off.end());
}

// rows[r] serves vectors a0 .. a0 + na against b0 .. b0 + nb (a diagonal row: the pairs i <= j of its block)
struct Span { int a0, na, b0, nb; bool diag; };

static void check_cover(const std::vector<Span> &rows, int n)
{
    std::vector<int> served((size_t)n * n, 0);
    for (const Span &s : rows) {
        CHECK(s.a0 >= 0 && s.na >= 1 && s.a0 + s.na <= n && s.b0 >= 0 && s.nb >= 1 && s.b0 + s.nb <= n);
        CHECK(s.diag == (s.a0 == s.b0) && (s.diag ? s.na == s.nb : s.a0 + s.na <= s.b0));
        if (s.a0 + s.na > n || s.b0 + s.nb > n) continue;
        for (int i = 0; i < s.na; i++)
            for (int j = s.diag ? i : 0; j < s.nb; j++) served[(size_t)(s.a0 + i) * n + s.b0 + j]++;
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) CHECK(served[(size_t)i * n + j] == (i <= j ? 1 : 0));
}

static void do_rows(int B, int HALF, int n)
{
    auto block_size = [&](int b) { return std::min(B, n - b * B); };
    {
        const kdbplan::Plan<GramRow> p = kdbplan::gram_plan<GramRow>(n, B);
        check_groups(p.groups, p.rows.size());
        std::vector<Span> spans;
        for (const kdbplan::Group &g : p.groups) {
            std::vector<int> all;
            for (int m = 1; m <= B; m++) all.push_back(m);
            check_inst(g, B, all);
            for (uint32_t r = g.row0; r < g.row0 + g.nrows && r < p.rows.size(); r++) {
                const GramRow &row = p.rows[r];
                CHECK(g.na == block_size(row.bi) && g.nb == block_size(row.bj) && g.diag == (row.bi == row.bj));
                spans.push_back(Span{row.bi * B, g.na, row.bj * B, g.nb, g.diag});
                printf("gram n=%d row=%u bi=%d bj=%d inst=%d,%d,%d\n", n, r, row.bi, row.bj, g.na, g.nb, (int)g.diag);
            }
        }
        check_cover(spans, n);
    }
    {
        const kdbplan::Plan<PairRow> p = kdbplan::pair_plan<PairRow>(n, B, HALF);
        check_groups(p.groups, p.rows.size());
        std::vector<Span> spans;
        for (const kdbplan::Group &g : p.groups) {
            check_inst(g, B, {1, HALF});
            for (uint32_t r = g.row0; r < g.row0 + g.nrows && r < p.rows.size(); r++) {
                const PairRow &row = p.rows[r];
                CHECK(g.na == row.na && g.nb == row.nb && g.diag == (row.a0 == row.b0));
                spans.push_back(Span{row.a0, row.na, row.b0, row.nb, g.diag});
                printf("pair n=%d row=%u a0=%d na=%d b0=%d nb=%d inst=%d,%d,%d\n", n, r, row.a0, row.na, row.b0, row.nb, g.na, g.nb, (int)g.diag);
            }
        }
        check_cover(spans, n);
        size_t off_groups = 0;
        for (const kdbplan::Group &g : p.groups) off_groups += !g.diag;
        CHECK(off_groups <= 2);                        // the rows of HALF vectors, then the rows of one
    }
    {
        const std::vector<FloatRow> rows = kdbplan::float_rows<FloatRow>(n);
        std::vector<int> served((size_t)n * n, 0);
        for (size_t r = 0; r < rows.size(); r++) {
            CHECK(rows[r].i < rows[r].j && rows[r].j < n);
            if (rows[r].j < n) served[(size_t)rows[r].i * n + rows[r].j]++;
            printf("float n=%d row=%zu i=%d j=%d\n", n, r, rows[r].i, rows[r].j);
        }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) CHECK(served[(size_t)i * n + j] == (i < j ? 1 : 0));
    }
}

static void print_list(const char *name, const std::vector<uint32_t> &v)
{
    printf(" %s=", name);
    for (size_t i = 0; i < v.size(); i++) printf(i ? ",%u" : "%u", v[i]);
}

static void do_score(int k, uint32_t piece, bool continues, uint64_t nbytes, const char *csv)
{
    // exactly sized: a read past the offsets is the sanitizer's to find
    std::vector<uint64_t> offs;
    for (const char *p = csv; *p;) {
        char *end = nullptr;
        offs.push_back(strtoull(p, &end, 10));
        p = *end == ',' ? end + 1 : end;
    }
    CHECK(offs.size() >= 2);
    const size_t nreads = offs.size() - 1;
    kdbplan::ScoreLayout lay;
    const kdbplan::LayoutError e = kdbplan::score_layout(offs.data(), nreads, nbytes, k, piece, continues, lay);
    CHECK(e == kdbplan::check_offsets(offs.data(), nreads, nbytes));
    printf("score k=%d continues=%d nbytes=%llu offs=%s:", k, (int)continues, (unsigned long long)nbytes, csv);
    if (e != kdbplan::LAYOUT_OK) {
        printf(" error=%s\n", e == kdbplan::LAYOUT_ENDS ? "ends" : "rise");
        CHECK(lay.rec_piece0.empty() && lay.piece_rec.empty() && lay.npieces == 0 && lay.nshort == 0);
        return;
    }
    CHECK(lay.rec_piece0.size() == nreads + 1 && lay.rec_piece0[0] == 0 && lay.rec_piece0[nreads] == lay.npieces && lay.npieces >= nreads);
    CHECK(lay.piece_rec.empty() || lay.piece_rec.size() == lay.npieces);
    for (size_t p = 0; p < lay.piece_rec.size(); p++)
        CHECK(lay.piece_rec[p] < nreads && lay.rec_piece0[lay.piece_rec[p]] <= p && p < lay.rec_piece0[lay.piece_rec[p] + 1]);
    printf(" nshort=%llu npieces=%llu", (unsigned long long)lay.nshort, (unsigned long long)lay.npieces);
    print_list("rec_piece0", lay.rec_piece0);
    print_list("piece_rec", lay.piece_rec);
    printf("\n");
}

int main(int argc, char **argv)
{
    auto num = [&](int i) { return strtoull(argv[i], nullptr, 10); };
    int i = 1;
    while (i < argc) {
        const std::string cmd = argv[i];
        if (cmd == "rows" && i + 3 < argc) {
            do_rows((int)num(i + 1), (int)num(i + 2), (int)num(i + 3));
            i += 4;
        } else if (cmd == "grid" && i + 5 < argc) {
            const kdbplan::Grid g = kdbplan::sweep_grid(num(i + 1), (uint32_t)num(i + 2), (uint32_t)num(i + 3), (uint32_t)num(i + 4), num(i + 5) != 0);
            CHECK(g.gx >= 1 && g.gx <= std::max<uint64_t>(1, num(i + 4)) && g.nparts == g.gx + 1);
            printf("grid nbins=%s cap=%s tail=%s: nchunks=%u gx=%u nparts=%u\n", argv[i + 1], argv[i + 4], argv[i + 5], g.nchunks, g.gx, g.nparts);
            i += 6;
        } else if (cmd == "cap" && i + 4 < argc) {
            printf("cap nrows=%s: %u\n", argv[i + 1], kdbplan::rows_cap((uint32_t)num(i + 1), (uint32_t)num(i + 2), (uint32_t)num(i + 3), (uint32_t)num(i + 4)));
            i += 5;
        } else if (cmd == "score" && i + 5 < argc) {
            do_score((int)num(i + 1), (uint32_t)num(i + 2), num(i + 3) != 0, num(i + 4), argv[i + 5]);
            i += 6;
        } else {
            printf("FAILED: command '%s' is unknown or short of arguments\n", argv[i]);
            return 2;
        }
    }
    if (bad) { printf("%d check(s) FAILED\n", bad); return 1; }
    printf("sweep plan check ok\n");
    return 0;
}
