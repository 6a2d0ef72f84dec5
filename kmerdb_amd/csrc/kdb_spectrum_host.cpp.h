// kdb_spectrum_host.cpp.h -- the host part of kdb_rank_transform (plain C++, no HIP: tests/c/spectrum_host_check.cpp compiles it alone and
// runs it under the sanitizers): from a vector's spectrum -- dense[v] = bins that hold v, for v < ndense, and the list of every larger value,
// once per occurrence -- to the tables rank_map_kernel looks its values up in.
//     rank2(v) = 2 below(v) + eq(v) + 1,   below(v) = bins that hold less than v, eq(v) = bins that hold v
// is twice the mid-rank of v: the eq(v) bins that hold v share the ranks below(v) + 1 ... below(v) + eq(v), whose mean is
// below(v) + (eq(v) + 1) / 2.  Summed over the N bins of a vector it gives N (N + 1), whatever the ties.
// Everything is uint64: below + eq <= N <= 2^36, so rank2 < 2^38 -- a dense entry above 2^32 (k = 17: nearly all of 2^34 bins are zero)
// is an ordinary case.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace kdbspectrum_host {

struct RankTables {
    std::vector<uint64_t> rank_dense;     // ndense entries: rank2(v); where no bin holds v, the value a bin holding v would get among the others (unused)
    std::vector<uint64_t> over_values;    // the distinct listed values, ascending
    std::vector<uint64_t> over_ranks;     // rank2 of each
    uint64_t nbins = 0;                   // Sum dense + n_over: the vector's length, for the caller to check
};

// `over` (n_over values, every one >= ndense, in any order) is sorted in place.
inline void rank_tables(const uint64_t *dense, uint64_t ndense, uint64_t *over, uint64_t n_over, RankTables &t)
{
    t.rank_dense.assign(ndense, 0);
    t.over_values.clear();
    t.over_ranks.clear();
    uint64_t below = 0;
    for (uint64_t v = 0; v < ndense; v++) {
        t.rank_dense[v] = 2 * below + dense[v] + 1;
        below += dense[v];
    }
    if (n_over) std::sort(over, over + n_over);
    for (uint64_t i = 0; i < n_over;) {
        uint64_t j = i + 1;
        while (j < n_over && over[j] == over[i]) j++;
        const uint64_t eq = j - i;
        t.over_values.push_back(over[i]);
        t.over_ranks.push_back(2 * below + eq + 1);
        below += eq;
        i = j;
    }
    t.nbins = below;
}

}  // namespace kdbspectrum_host
