// The direction scratch of kdb_align_traceback and the chunks it works through (kdbplan::align_trace_bytes / align_trace_chunks of
// kmerdb_amd/csrc/kdb_sweep_plan.cpp.h) alone, for AddressSanitizer + UBSan on the CPU.  Every command of the command line is one of:
//     bytes m n d band                             one task: an oriented query of m residues, a record of n, the diagonal d
//     chunks limit b,b,..                          a batch of tasks by their bytes ("-" = no tasks)
// It checks a task's bytes against a brute-force count of the groups of steps its band's cells fall into and every cell's dword against
// those bytes, the chunks against what the header promises of them, and prints for tests/test_traceback_plan_host.py to compare:
//     bytes empty=0|1 groups=.. bytes=.. brute=..
//     chunks n=.. largest=.. bytes=.. first=a,b,..
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o traceback_plan_check tests/c/traceback_plan_check.cpp && ./traceback_plan_check bytes 150 5000 -20 16
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kmerdb_amd/csrc/kdb_sweep_plan.cpp.h"

static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); bad++; } } while (0)

static std::vector<unsigned long long> numbers(const char *s)
{
    std::vector<unsigned long long> v;
    if (!strcmp(s, "-")) return v;
    for (const char *p = s; *p;) {
        char *end = nullptr;
        v.push_back(strtoull(p, &end, 10));
        p = *end ? end + 1 : end;
    }
    return v;
}

static void do_bytes(uint64_t m, uint64_t n, int64_t d, uint32_t band)
{
    const kdbplan::AlignWindow w = kdbplan::align_window(m, n, d, band);
    const uint32_t groups = kdbplan::align_trace_groups(w, band);
    const uint64_t bytes = kdbplan::align_trace_bytes(w, band);
    // brute force: the steps T = i + c / 2 of every cell of the band in the rows that hold a cell of the record, and the groups of
    // ALIGN_GROUP steps (they begin at multiples of ALIGN_GROUP) that hold one
    uint64_t brute = 0;
    if (!w.empty()) {
        const uint32_t t_lo = kdbplan::align_t_lo(w);
        std::vector<bool> group_used(((uint64_t)m + 2 * band) / kdbplan::ALIGN_GROUP + 2, false);
        for (uint64_t i = 0; i < m; i++) {
            bool in_record = false;
            for (uint32_t c = 0; c <= 2 * band && !in_record; c++) {
                const int64_t j = (int64_t)i + w.jb + c;
                in_record = j >= 0 && j < (int64_t)n;
            }
            if (!in_record) continue;
            for (uint32_t c = 0; c <= 2 * band; c++) {
                const uint64_t T = i + c / 2;
                group_used[T / kdbplan::ALIGN_GROUP] = true;
                // the cell's dword lies inside the task's bytes
                CHECK(T >= t_lo);
                const uint64_t dword = kdbplan::align_trace_dword((uint32_t)((T - t_lo) / kdbplan::ALIGN_GROUP), c / 2);
                if (!(4 * dword + 4 <= bytes)) { CHECK(4 * dword + 4 <= bytes); break; }
            }
        }
        for (bool used : group_used) brute += used ? 1 : 0;
        // the last lane's dword of the last group is the last of the bytes
        CHECK(4 * kdbplan::align_trace_dword(groups - 1, kdbplan::ALIGN_LANES - 1) + 4 == bytes);
    }
    printf("bytes empty=%d groups=%u bytes=%llu brute=%llu\n", w.empty() ? 1 : 0, groups, (unsigned long long)bytes, (unsigned long long)brute);
    CHECK(bytes == (uint64_t)groups * 4 * kdbplan::ALIGN_LANES && bytes % 256 == 0);
    CHECK(groups == brute);
}

static void do_chunks(uint64_t limit, const std::vector<unsigned long long> &b)
{
    std::vector<uint64_t> bytes(b.begin(), b.end());
    kdbplan::AlignTraceChunks ch;
    kdbplan::align_trace_chunks(bytes.data(), bytes.size(), limit, ch);
    const size_t n = bytes.size(), nchunks = ch.first.empty() ? 0 : ch.first.size() - 1;
    CHECK(ch.offs.size() == n);
    if (n == 0) CHECK(nchunks == 0 && ch.largest == 0 && ch.bytes == 0);
    else CHECK(nchunks >= 1 && ch.first.front() == 0 && ch.first.back() == n);
    // every task lies in exactly one chunk, the chunks are consecutive and none is empty; a chunk is within the limit unless it is a
    // single task; it is the longest run that fits: the next task would not; the offsets are the sums of the bytes before, per chunk
    uint64_t largest = 0, sum = 0;
    std::vector<int> seen(n, 0);
    for (size_t k = 0; k < nchunks; k++) {
        const uint64_t lo = ch.first[k], hi = ch.first[k + 1];
        CHECK(lo < hi && hi <= n);
        uint64_t used = 0;
        for (uint64_t t = lo; t < hi && t < n; t++) {
            seen[t]++;
            CHECK(ch.offs[t] == used);
            used += bytes[t];
        }
        CHECK(used <= limit || hi - lo == 1);
        if (hi < n) CHECK(used > limit || bytes[hi] > limit - used);
        largest = std::max(largest, used);
        sum += used;
    }
    for (size_t t = 0; t < n; t++) CHECK(seen[t] == 1);
    CHECK(largest == ch.largest && sum == ch.bytes);
    printf("chunks n=%zu largest=%llu bytes=%llu first=", nchunks, (unsigned long long)ch.largest, (unsigned long long)ch.bytes);
    for (size_t k = 0; k < ch.first.size(); k++) printf("%s%llu", k ? "," : "", (unsigned long long)ch.first[k]);
    printf("\n");
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc;) {
        if (!strcmp(argv[i], "bytes") && i + 4 < argc) {
            do_bytes(strtoull(argv[i + 1], nullptr, 10), strtoull(argv[i + 2], nullptr, 10), strtoll(argv[i + 3], nullptr, 10), (uint32_t)atoi(argv[i + 4]));
            i += 5;
        } else if (!strcmp(argv[i], "chunks") && i + 2 < argc) {
            do_chunks(strtoull(argv[i + 1], nullptr, 10), numbers(argv[i + 2]));
            i += 3;
        } else {
            printf("FAILED unknown command %s\n", argv[i]);
            return 2;
        }
    }
    if (bad) return 1;
    printf("traceback plan check ok\n");
    return 0;
}
