// The piece layout of kdb_record_tables (kdbplan::tables_layout of kmerdb_amd/csrc/kdb_sweep_plan.cpp.h) alone, for AddressSanitizer +
// UBSan on the CPU.  Every command of the command line is one layout:
//     tables k stride phase piece max_entries nbytes o,o,..     the records with the offsets o,.. in nbytes residues
// It checks the layout's own invariants and prints it for tests/test_tables_plan_host.py to compare with tests/tables_cases.py:
//     layout npieces=.. multi=r,r,.. piece_rec=0|1            (or: refused ends | rise | entries)
//     piece p=.. rec=.. first=.. count=.. at=..                the windows [first, first + count) of the record, the first one at residue `at` of the batch
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o tables_plan_check tests/c/tables_plan_check.cpp && ./tables_plan_check tables 3 3 0 8 64 9 0,9
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kmerdb_amd/csrc/kdb_sweep_plan.cpp.h"

static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); bad++; } } while (0)

static std::vector<uint64_t> numbers(const char *s)
{
    std::vector<uint64_t> v;
    for (const char *p = s; *p;) {
        char *end = nullptr;
        v.push_back(strtoull(p, &end, 10));
        p = *end ? end + 1 : end;
    }
    return v;
}

static void do_tables(int k, int stride, uint64_t phase, uint32_t piece, uint64_t max_entries, uint64_t nbytes, const std::vector<uint64_t> &offs)
{
    const size_t nreads = offs.size() - 1;
    kdbplan::TablesLayout lay;
    const kdbplan::LayoutError e = kdbplan::tables_layout(offs.data(), nreads, nbytes, k, stride, phase, piece, max_entries, lay);
    // the offsets are judged first, the entries after them
    CHECK(kdbplan::check_offsets(offs.data(), nreads, nbytes) == (e == kdbplan::LAYOUT_ENTRIES ? kdbplan::LAYOUT_OK : e));
    if (e != kdbplan::LAYOUT_OK) {
        printf("refused %s\n", e == kdbplan::LAYOUT_ENDS ? "ends" : e == kdbplan::LAYOUT_RISE ? "rise" : "entries");
        CHECK(lay.rec_piece0.empty() && lay.piece_rec.empty() && lay.multi.empty() && lay.npieces == 0);
        return;
    }
    CHECK(lay.rec_piece0.size() == nreads + 1 && lay.rec_piece0[0] == 0 && lay.rec_piece0[nreads] == lay.npieces);
    CHECK(lay.piece_rec.empty() ? lay.multi.empty() && lay.npieces == nreads : lay.piece_rec.size() == lay.npieces && !lay.multi.empty());
    printf("layout npieces=%llu multi=", (unsigned long long)lay.npieces);
    for (size_t i = 0; i < lay.multi.size(); i++) printf("%s%u", i ? "," : "", lay.multi[i]);
    printf(" piece_rec=%d\n", lay.piece_rec.empty() ? 0 : 1);
    size_t m = 0;
    for (size_t r = 0; r < nreads; r++) {
        const uint64_t ph = r == 0 ? phase : 0, len = offs[r + 1] - offs[r];
        const uint64_t nwin = kdbplan::tables_windows(len, k, stride, ph);
        const uint32_t p0 = lay.rec_piece0[r], p1 = lay.rec_piece0[r + 1];
        CHECK(p1 > p0);
        CHECK((p1 - p0 > 1) == (m < lay.multi.size() && lay.multi[m] == r));
        if (p1 - p0 > 1) m++;
        uint64_t covered = 0;
        for (uint32_t p = p0; p < p1; p++) {
            if (!lay.piece_rec.empty()) CHECK(lay.piece_rec[p] == r);
            uint64_t first = 0;
            uint32_t count = 0;
            kdbplan::TablesLayout::piece_windows(nwin, p - p0, piece, first, count);
            CHECK(first == covered && count <= piece && (count > 0 || nwin == 0));
            CHECK(p + 1 == p1 || count == piece);
            // every residue a counted window of the piece reads lies inside the record
            if (count) CHECK(ph + (first + count - 1) * (uint64_t)stride + (uint64_t)k <= len);
            covered += count;
            printf("piece p=%u rec=%zu first=%llu count=%u at=%llu\n", p, r, (unsigned long long)first, count,
                   (unsigned long long)(offs[r] + ph + first * (uint64_t)stride));
        }
        CHECK(covered == nwin);
        // one more window would pass the record's end
        CHECK(ph + nwin * (uint64_t)stride + (uint64_t)k > len);
    }
    CHECK(m == lay.multi.size());
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc;) {
        if (!strcmp(argv[i], "tables") && i + 7 < argc) {
            do_tables(atoi(argv[i + 1]), atoi(argv[i + 2]), strtoull(argv[i + 3], nullptr, 10), (uint32_t)strtoul(argv[i + 4], nullptr, 10),
                      strtoull(argv[i + 5], nullptr, 10), strtoull(argv[i + 6], nullptr, 10), numbers(argv[i + 7]));
            i += 8;
        } else {
            printf("FAILED unknown command %s\n", argv[i]);
            return 2;
        }
    }
    if (bad) return 1;
    printf("tables plan check ok\n");
    return 0;
}
