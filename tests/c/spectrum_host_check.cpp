// The host part of kdb_rank_transform (kmerdb_amd/csrc/kdb_spectrum_host.cpp.h) alone, for AddressSanitizer + UBSan on the CPU: rank tables
// from a dense table plus a list of large values, against ranks counted the slow way.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o spectrum_host_check tests/c/spectrum_host_check.cpp && ./spectrum_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../kmerdb_amd/csrc/kdb_spectrum_host.cpp.h"

static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); bad++; } } while (0)

// a whole vector: its spectrum, its tables, and every bin's rank against a count over all bins
static void check_vector(const std::vector<uint64_t> &x, uint64_t ndense)
{
    std::vector<uint64_t> dense(ndense, 0), over;
    for (uint64_t v : x) { if (v < ndense) dense[v]++; else over.push_back(v); }
    // exactly sized buffers: a read or write past either end is the sanitizer's to find
    std::vector<uint64_t> list(over);
    kdbspectrum_host::RankTables t;
    kdbspectrum_host::rank_tables(dense.data(), ndense, list.data(), list.size(), t);
    CHECK(t.nbins == x.size());
    CHECK(t.rank_dense.size() == ndense && t.over_values.size() == t.over_ranks.size());
    for (size_t i = 1; i < t.over_values.size(); i++) CHECK(t.over_values[i - 1] < t.over_values[i]);
    unsigned __int128 sum = 0;
    for (uint64_t v : x) {
        uint64_t below = 0, eq = 0;
        for (uint64_t w : x) { below += w < v; eq += w == v; }
        uint64_t got;
        if (v < ndense) got = t.rank_dense[v];
        else {
            const auto it = std::lower_bound(t.over_values.begin(), t.over_values.end(), v);
            CHECK(it != t.over_values.end() && *it == v);
            got = it == t.over_values.end() ? 0 : t.over_ranks[it - t.over_values.begin()];
        }
        CHECK(got == 2 * below + eq + 1);
        sum += got;
    }
    CHECK(sum == (unsigned __int128)x.size() * (x.size() + 1));
}

int main()
{
    const uint64_t U64_MAX = ~0ull;
    // an empty list, with and without empty dense entries
    check_vector({0, 0, 0, 1, 5, 5, 2}, 8);
    check_vector({3}, 4);
    check_vector({7, 7, 7, 7}, 8);
    // duplicates in the list, 2^64 - 1, values right at the table's end
    check_vector({0, 9, 8, 8, 7, 100, 100, 100, U64_MAX, U64_MAX, 1ull << 40, 8, 0}, 8);
    check_vector({U64_MAX}, 8);
    check_vector({U64_MAX, U64_MAX, U64_MAX}, 8);
    check_vector({8, 9, 10, 11}, 8);                                       // nothing in the table at all
    // random vectors with many ties, the real table size
    std::mt19937_64 rng(5);
    for (int round = 0; round < 6; round++) {
        std::vector<uint64_t> x(300 + 97 * round);
        for (auto &v : x) {
            const uint64_t r = rng() % 100;
            v = r < 60 ? rng() % 4 : r < 90 ? rng() % 70000 : r < 97 ? 65536 + rng() % 5 : rng() | (1ull << 63);
        }
        check_vector(x, round % 2 ? 65536 : 16);
    }
    // a dense entry above 2^32 (k = 17: nearly all of 2^34 bins are zero) and the ranks behind it, from a table written down directly
    {
        std::vector<uint64_t> dense(65536, 0), list = {70000, U64_MAX, 70000};
        dense[0] = (1ull << 34) - 10;
        dense[1] = 6;
        dense[65535] = 1;
        kdbspectrum_host::RankTables t;
        kdbspectrum_host::rank_tables(dense.data(), dense.size(), list.data(), list.size(), t);
        const uint64_t n0 = dense[0];
        CHECK(t.nbins == (1ull << 34));
        CHECK(t.rank_dense[0] == n0 + 1);
        CHECK(t.rank_dense[1] == 2 * n0 + 6 + 1);
        CHECK(t.rank_dense[65535] == 2 * (n0 + 6) + 1 + 1);
        CHECK(t.over_values.size() == 2 && t.over_values[0] == 70000 && t.over_values[1] == U64_MAX);
        CHECK(t.over_ranks[0] == 2 * (n0 + 7) + 2 + 1 && t.over_ranks[1] == 2 * (n0 + 9) + 1 + 1);
        // Sum over the bins of rank2 = N (N + 1), in 128 bits
        unsigned __int128 sum = (unsigned __int128)n0 * t.rank_dense[0] + (unsigned __int128)6 * t.rank_dense[1] + t.rank_dense[65535] + 2 * (unsigned __int128)t.over_ranks[0] + t.over_ranks[1];
        CHECK(sum == (unsigned __int128)t.nbins * (t.nbins + 1));
    }
    // no list at all: a NULL pointer with zero entries must not be touched
    {
        std::vector<uint64_t> dense = {2, 0, 1};
        kdbspectrum_host::RankTables t;
        kdbspectrum_host::rank_tables(dense.data(), dense.size(), nullptr, 0, t);
        CHECK(t.nbins == 3 && t.over_values.empty() && t.rank_dense[0] == 3 && t.rank_dense[2] == 6);
    }
    if (bad) { printf("%d checks failed\n", bad); return 1; }
    printf("spectrum host check ok\n");
    return 0;
}
