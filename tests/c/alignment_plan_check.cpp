// The task windows and the batch layout of kdb_align_banded (kdbplan::align_window / align_layout of kmerdb_amd/csrc/kdb_sweep_plan.cpp.h)
// alone, for AddressSanitizer + UBSan on the CPU.  Every command of the command line is one of:
//     window m n d band stage                      one task: an oriented query of m residues, a record of n, the diagonal d
//     layout band max_query waves grid_max q_nbytes qo,qo,.. r_nbytes ro,ro,.. tq,.. tr,.. d,.. strand,..      a batch ("-" = no tasks)
// It checks the window against a brute-force walk over the band's cells, the LDS a stage of the kernel reads against what it stages, and
// prints for tests/test_alignment_plan_host.py to compare with the definition:
//     window empty=0|1 r_lo=.. r_hi=.. i_lo=.. i_hi=.. jb=.. t_lo=.. t_hi=.. stages=.. lds_wave=..
//     layout grid=.. cells=.. nonempty=..          (or: refused ends | rise | task t | strand t | query t)
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o alignment_plan_check tests/c/alignment_plan_check.cpp && ./alignment_plan_check window 150 5000 -20 16 512
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kmerdb_amd/csrc/kdb_sweep_plan.cpp.h"

static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); bad++; } } while (0)

static std::vector<long long> numbers(const char *s)
{
    std::vector<long long> v;
    if (!strcmp(s, "-")) return v;
    for (const char *p = s; *p;) {
        char *end = nullptr;
        v.push_back(strtoll(p, &end, 10));
        p = *end ? end + 1 : end;
    }
    return v;
}

static void do_window(uint64_t m, uint64_t n, int64_t d, uint32_t band, uint32_t stage)
{
    const kdbplan::AlignWindow w = kdbplan::align_window(m, n, d, band);
    const uint32_t t_lo = kdbplan::align_t_lo(w), t_hi = w.empty() ? 0 : kdbplan::align_t_hi(w, band), stages = kdbplan::align_stages(w, band, stage);
    printf("window empty=%d r_lo=%u r_hi=%u i_lo=%u i_hi=%u jb=%d t_lo=%u t_hi=%u stages=%u lds_wave=%u\n", w.empty() ? 1 : 0, w.r_lo, w.r_hi, w.i_lo, w.i_hi, w.jb, t_lo,
           t_hi, stages, kdbplan::align_lds_wave(stage));
    CHECK(kdbplan::align_lds_wave(stage) % 8 == 0 && kdbplan::align_lds_q(stage) % 4 == 0);
    if (w.empty()) {
        CHECK(w.r_lo == 0 && w.r_hi == 0 && w.i_lo == 0 && w.i_hi == 0 && w.jb == 0 && stages == 0);
    } else {
        CHECK((int64_t)w.jb == d - (int64_t)band && w.i_hi <= m && w.r_hi <= n && w.r_lo < w.r_hi);
        CHECK(t_lo % kdbplan::ALIGN_GROUP == 0 && t_lo <= w.i_lo && w.i_lo - t_lo < kdbplan::ALIGN_GROUP && stages >= 1);
        CHECK((uint64_t)t_lo + (uint64_t)stages * stage >= t_hi && (uint64_t)t_lo + (uint64_t)(stages - 1) * stage < t_hi);
    }
    // brute force, where the matrix is small: the rows and the columns that hold a cell in band
    if (m <= 4096 && (d > -100000 && d < 100000)) {
        int64_t i_lo = -1, i_hi = -1, r_lo = -1, r_hi = -1;
        for (int64_t i = 0; i < (int64_t)m; i++)
            for (int64_t c = 0; c <= 2 * (int64_t)band; c++) {
                const int64_t j = i + d - (int64_t)band + c;
                if (j < 0 || j >= (int64_t)n) continue;
                if (i_lo < 0) i_lo = i;
                i_hi = i + 1;
                if (r_lo < 0 || j < r_lo) r_lo = j;
                if (j + 1 > r_hi) r_hi = j + 1;
            }
        CHECK(w.empty() == (i_lo < 0));
        if (!w.empty() && i_lo >= 0) CHECK(w.i_lo == i_lo && w.i_hi == i_hi && w.r_lo == r_lo && w.r_hi == r_hi);
    }
    if (w.empty()) return;
    // what the kernel reads in every group of every stage, for every lane, lies in what the stage holds (LDS bytes), and the staged rows and
    // columns cover every cell of the window the lane computes there
    const uint32_t L = kdbplan::ALIGN_LANES, G = kdbplan::ALIGN_GROUP, lds_q = kdbplan::align_lds_q(stage), lds_r = kdbplan::align_lds_r(stage);
    for (uint32_t s = 0; s < stages; s++) {
        if (s >= 2 && s + 2 < stages) continue;                                // (the first and the last stages of a long task)
        const uint32_t ts = t_lo + s * stage, t_end = std::min(ts + stage, t_hi);
        for (uint32_t t0 = ts; t0 < t_end; t0 += G) {
            for (uint32_t lane = 0; lane < L; lane++) {
                const uint32_t x = (t0 - ts) + L - lane, y = x + 2 * lane;
                CHECK(x >= 1 && (x / 4 + 2) * 4 <= lds_q);                     // two aligned words around x .. x + 3
                CHECK((y / 4 + 2) * 4 <= lds_r && y + 4 < (y / 4 + 2) * 4);    // ... and around y .. y + 4
                // byte x is row ts - L + x = t0 - lane: the lane's first row of the group
                CHECK((int64_t)ts - L + x == (int64_t)t0 - lane);
                // byte y is column ts - L + jb + y = row + 2 lane + jb: the lane's even diagonal in that row
                CHECK((int64_t)ts - L + w.jb + y == (int64_t)t0 - lane + 2 * lane + w.jb);
            }
        }
    }
    CHECK(kdbplan::align_t_hi(w, band) - 1 - band == w.i_hi - 1);                  // the last step's lane `band` is on the last row
}

static void do_layout(char **a)
{
    const uint32_t band = (uint32_t)atoi(a[0]), waves = (uint32_t)atoi(a[2]), grid_max = (uint32_t)atoi(a[3]);
    const uint64_t max_query = strtoull(a[1], nullptr, 10), q_nbytes = strtoull(a[4], nullptr, 10), r_nbytes = strtoull(a[6], nullptr, 10);
    std::vector<uint64_t> qo, ro;
    for (long long v : numbers(a[5])) qo.push_back((uint64_t)v);
    for (long long v : numbers(a[7])) ro.push_back((uint64_t)v);
    std::vector<uint32_t> tq, tr;
    std::vector<int64_t> td;
    std::vector<uint8_t> st;
    for (long long v : numbers(a[8])) tq.push_back((uint32_t)v);
    for (long long v : numbers(a[9])) tr.push_back((uint32_t)v);
    for (long long v : numbers(a[10])) td.push_back((int64_t)v);
    for (long long v : numbers(a[11])) st.push_back((uint8_t)v);
    CHECK(tq.size() == tr.size() && tq.size() == td.size() && tq.size() == st.size() && !qo.empty() && !ro.empty());
    kdbplan::AlignLayout lay;
    const kdbplan::LayoutError e = kdbplan::align_layout(qo.data(), qo.size() - 1, q_nbytes, ro.data(), ro.size() - 1, r_nbytes, tq.data(), tr.data(), td.data(), st.data(),
                                                         tq.size(), band, max_query, waves, grid_max, lay);
    if (e != kdbplan::LAYOUT_OK) {
        CHECK(lay.grid == 0 && lay.cells == 0);
        if (e == kdbplan::LAYOUT_ENDS || e == kdbplan::LAYOUT_RISE) printf("refused %s\n", e == kdbplan::LAYOUT_ENDS ? "ends" : "rise");
        else printf("refused %s %llu\n", e == kdbplan::LAYOUT_TASK ? "task" : e == kdbplan::LAYOUT_STRAND ? "strand" : "query", (unsigned long long)lay.bad);
        return;
    }
    CHECK(lay.grid >= 1 && lay.grid <= grid_max && (uint64_t)lay.grid * waves >= std::min<uint64_t>(tq.size(), (uint64_t)grid_max * waves));
    CHECK(tq.empty() || (uint64_t)(lay.grid - 1) * waves < tq.size());
    printf("layout grid=%u cells=%llu nonempty=%llu\n", lay.grid, (unsigned long long)lay.cells, (unsigned long long)lay.nonempty);
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc;) {
        if (!strcmp(argv[i], "window") && i + 5 < argc) {
            do_window(strtoull(argv[i + 1], nullptr, 10), strtoull(argv[i + 2], nullptr, 10), strtoll(argv[i + 3], nullptr, 10), (uint32_t)atoi(argv[i + 4]),
                      (uint32_t)atoi(argv[i + 5]));
            i += 6;
        } else if (!strcmp(argv[i], "layout") && i + 12 < argc) {
            do_layout(argv + i + 1);
            i += 13;
        } else {
            printf("FAILED unknown command %s\n", argv[i]);
            return 2;
        }
    }
    if (bad) return 1;
    printf("alignment plan check ok\n");
    return 0;
}
