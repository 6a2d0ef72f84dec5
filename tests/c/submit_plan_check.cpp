// The cut of a submit into staging pieces (kdbplan::SubmitCutter of kmerdb_amd/csrc/kdb_submit_plan.cpp.h) alone, for AddressSanitizer +
// UBSan on the CPU.  Every command of the command line is one submit:
//     submit cap max_recs k first_continues nbytes o,o,..      the records with the offsets o,.. in a buffer of nbytes
// It checks the pieces' own invariants and prints them for tests/test_submit_plan_host.py to compare with tests/submit_cases.py:
//     submit                                                     (one per command, then its pieces)
//     piece start=.. nbytes=.. rec0=.. nrecs=.. cont=0|1 inside=0|1 local=0,..
//     refused ends|rise at=.. text=..                            (the engine's message; what was cut before it stays printed)
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o submit_plan_check tests/c/submit_plan_check.cpp && ./submit_plan_check submit 64 3 5 0 65 0,65
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kmerdb_amd/csrc/kdb_submit_plan.cpp.h"

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

static void do_submit(uint64_t cap, size_t max_recs, int k, bool first_continues, uint64_t nbytes, const std::vector<uint64_t> &offs)
{
    const size_t nreads = offs.size() - 1;
    printf("submit\n");
    if (kdbplan::SubmitCutter::check_ends(offs.data(), nreads, nbytes) != kdbplan::SUBMIT_OK) {
        printf("refused ends at=0 text=%s\n", kdbplan::SUBMIT_ENDS_TEXT);
        return;
    }
    kdbplan::SubmitCutter cut(offs.data(), nreads, first_continues, cap, max_recs, k);
    size_t npieces = 0;
    while (!cut.done()) {
        std::vector<uint64_t> local(max_recs + 1, ~0ull);           // (exactly what the cutter may write: the sanitizer sees one entry more)
        kdbplan::SubmitPiece p;
        if (cut.next(local.data(), p) != kdbplan::SUBMIT_OK) {
            char text[128];
            snprintf(text, sizeof text, kdbplan::SUBMIT_RISE_FORMAT, cut.bad);
            printf("refused rise at=%zu text=%s\n", cut.bad, text);
            return;
        }
        CHECK(p.nrecs >= 1 && p.nrecs <= max_recs && p.nbytes <= cap);
        CHECK(p.rec0 + p.nrecs <= nreads && p.start + p.nbytes <= offs[nreads]);
        CHECK(local[0] == 0 && local[p.nrecs] == p.nbytes);
        for (size_t i = 1; i <= p.nrecs; i++) CHECK(local[i] >= local[i - 1]);
        CHECK(!p.ends_inside_record || (p.nrecs == 1 && p.nbytes == cap));
        CHECK((npieces == 0 && !first_continues) ? !p.first_is_continuation : true);
        printf("piece start=%llu nbytes=%llu rec0=%zu nrecs=%zu cont=%d inside=%d local=", (unsigned long long)p.start, (unsigned long long)p.nbytes, p.rec0,
               p.nrecs, p.first_is_continuation ? 1 : 0, p.ends_inside_record ? 1 : 0);
        for (size_t i = 0; i <= p.nrecs; i++) printf("%s%llu", i ? "," : "", (unsigned long long)local[i]);
        printf("\n");
        npieces++;
        if (npieces > 4 * (nreads + offs[nreads] / (cap - (uint64_t)(k - 1)) + 1)) { CHECK(!"the cut does not end"); return; }
    }
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc;) {
        if (!strcmp(argv[i], "submit") && i + 6 < argc) {
            do_submit(strtoull(argv[i + 1], nullptr, 10), (size_t)strtoull(argv[i + 2], nullptr, 10), atoi(argv[i + 3]), atoi(argv[i + 4]) != 0,
                      strtoull(argv[i + 5], nullptr, 10), numbers(argv[i + 6]));
            i += 7;
        } else {
            printf("FAILED unknown command %s\n", argv[i]);
            return 2;
        }
    }
    if (bad) return 1;
    printf("submit plan check ok\n");
    return 0;
}
