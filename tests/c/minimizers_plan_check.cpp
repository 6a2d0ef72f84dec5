// The piece layout of kdb_minimizers (kdbplan::minimizers_layout of kmerdb_amd/csrc/kdb_sweep_plan.cpp.h) alone, for AddressSanitizer +
// UBSan on the CPU.  Every command of the command line is one layout:
//     minimizers k w piece nbytes o,o,..          the records with the offsets o,.. in nbytes residues
// It checks the layout's own invariants and prints it for tests/test_minimizers_plan_host.py to compare with the definition:
//     layout npieces=.. max_keys=.. lds_wave=.. piece_rec=0|1        (or: refused ends | rise)
//     piece p=.. rec=.. first=.. count=.. lo=.. hi=..                  the piece owns the start positions [first, first + count) and reads the keys of [lo, hi)
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o minimizers_plan_check tests/c/minimizers_plan_check.cpp && ./minimizers_plan_check minimizers 3 2 8 9 0,9
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

static void do_minimizers(int k, uint32_t w, uint32_t piece, uint64_t nbytes, const std::vector<uint64_t> &offs)
{
    const size_t nreads = offs.size() - 1;
    kdbplan::MinimizersLayout lay;
    const kdbplan::LayoutError e = kdbplan::minimizers_layout(offs.data(), nreads, nbytes, k, w, piece, lay);
    CHECK(e == kdbplan::check_offsets(offs.data(), nreads, nbytes));
    if (e != kdbplan::LAYOUT_OK) {
        printf("refused %s\n", e == kdbplan::LAYOUT_ENDS ? "ends" : "rise");
        CHECK(lay.rec_piece0.empty() && lay.piece_rec.empty() && lay.npieces == 0 && lay.max_keys == 0 && lay.lds_wave == 0);
        return;
    }
    CHECK(lay.rec_piece0.size() == nreads + 1 && lay.rec_piece0[0] == 0 && lay.rec_piece0[nreads] == lay.npieces);
    CHECK(lay.piece_rec.empty() ? lay.npieces == nreads : lay.piece_rec.size() == lay.npieces && lay.npieces > nreads);
    CHECK(lay.lds_wave % 8 == 0);
    printf("layout npieces=%llu max_keys=%u lds_wave=%u piece_rec=%d\n", (unsigned long long)lay.npieces, lay.max_keys, lay.lds_wave, lay.piece_rec.empty() ? 0 : 1);
    uint32_t widest = 0;
    for (size_t r = 0; r < nreads; r++) {
        const uint64_t len = offs[r + 1] - offs[r], nwin = kdbplan::minimizer_positions(len, k);
        const uint32_t p0 = lay.rec_piece0[r], p1 = lay.rec_piece0[r + 1];
        CHECK(p1 > p0);
        CHECK(nwin == 0 ? len < (uint64_t)k : nwin + (uint64_t)k - 1 == len);
        uint64_t covered = 0;
        for (uint32_t p = p0; p < p1; p++) {
            if (!lay.piece_rec.empty()) CHECK(lay.piece_rec[p] == r);
            const kdbplan::MinimizerPiece pc = kdbplan::minimizer_piece(nwin, p - p0, piece, w);
            CHECK(pc.first == covered && pc.count <= piece && (pc.count > 0 || nwin == 0));
            CHECK(p + 1 == p1 || pc.count == piece);
            CHECK(pc.lo <= pc.first && pc.first + pc.count <= pc.hi && pc.hi <= nwin);
            if (pc.count) {
                // w - 1 positions on either side, or as many as the record has; the residues behind the keys lie inside the record
                CHECK(pc.first - pc.lo == std::min<uint64_t>(w - 1, pc.first));
                CHECK(pc.hi - (pc.first + pc.count) == std::min<uint64_t>(w - 1, nwin - (pc.first + pc.count)));
                CHECK(pc.hi + (uint64_t)k - 1 <= len);
                // what the kernel stages: whole 4-byte words around the residues [lo, hi + k - 1) of the record, behind the keys in the wave's LDS
                const uint64_t r0 = offs[r] + pc.lo, a0 = r0 & ~(uint64_t)3;
                const uint64_t words = (r0 - a0 + (pc.hi - pc.lo) + (uint64_t)k - 1 + 3) / 4;
                CHECK((uint64_t)lay.max_keys * 8 + words * 4 <= lay.lds_wave);
                CHECK(a0 + words * 4 <= nbytes + 3);
            } else {
                CHECK(pc.lo == pc.hi);
            }
            CHECK(pc.hi - pc.lo <= lay.max_keys);
            widest = std::max(widest, (uint32_t)(pc.hi - pc.lo));
            covered += pc.count;
            // the emit pass asks for the same piece with w = 1: the same own positions
            const kdbplan::MinimizerPiece own = kdbplan::minimizer_piece(nwin, p - p0, piece, 1);
            CHECK(own.first == pc.first && own.count == pc.count && own.lo == pc.first && own.hi == pc.first + pc.count);
            printf("piece p=%u rec=%zu first=%llu count=%u lo=%llu hi=%llu\n", p, r, (unsigned long long)pc.first, pc.count, (unsigned long long)pc.lo,
                   (unsigned long long)pc.hi);
        }
        CHECK(covered == nwin);
    }
    CHECK(widest == lay.max_keys);
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc;) {
        if (!strcmp(argv[i], "minimizers") && i + 5 < argc) {
            do_minimizers(atoi(argv[i + 1]), (uint32_t)strtoul(argv[i + 2], nullptr, 10), (uint32_t)strtoul(argv[i + 3], nullptr, 10),
                          strtoull(argv[i + 4], nullptr, 10), numbers(argv[i + 5]));
            i += 6;
        } else {
            printf("FAILED unknown command %s\n", argv[i]);
            return 2;
        }
    }
    if (bad) return 1;
    printf("minimizers plan check ok\n");
    return 0;
}
