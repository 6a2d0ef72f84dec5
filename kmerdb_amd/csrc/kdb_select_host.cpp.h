// kdb_select_host.cpp.h -- what the radix select of kdb_size_factors shares between the device and the host (plain C++; under hipcc the key
// transform is __host__ __device__; tests/c/select_host_check.cpp compiles this file alone with g++ and runs it under the sanitizers).
//
// A float64 maps to a uint64 key that orders like the value: the sign bit is flipped, and for negatives all other bits too.  -0.0 sorts
// directly below +0.0; nan never reaches the select (ineligible bins carry it as their marker and are skipped).
//
// The select goes through the key from the top, one digit per pass: NPASS = 6 digits of 11, 11, 11, 11, 11 and 9 bits.  A pass histograms
// the digit at `shift` among the elements whose bits above the digit equal the prefix chosen so far; narrow() takes that histogram and the
// wanted rank (0-based, among the elements under the prefix) to the digit's bucket and the rank inside it.  The median of an even number of
// elements needs two neighbouring ranks, which share their prefix up to some digit and then part: Select carries up to two
// (prefix, rank) targets and splits the first time the two ranks fall in different buckets.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define KDB_SELECT_HD __host__ __device__
#else
#define KDB_SELECT_HD
#endif

namespace kdbselect {

constexpr int DIGIT_BITS = 11;
constexpr int NBUCKET = 1 << DIGIT_BITS;
constexpr int NPASS = (64 + DIGIT_BITS - 1) / DIGIT_BITS;

KDB_SELECT_HD inline int pass_shift(int pass) { const int s = 64 - DIGIT_BITS * (pass + 1); return s < 0 ? 0 : s; }
KDB_SELECT_HD inline int pass_width(int pass) { const int s = 64 - DIGIT_BITS * (pass + 1); return s < 0 ? DIGIT_BITS + s : DIGIT_BITS; }

KDB_SELECT_HD inline uint64_t key_of_bits(uint64_t bits) { return (bits >> 63) ? ~bits : (bits | (1ull << 63)); }
KDB_SELECT_HD inline uint64_t bits_of_key(uint64_t key) { return (key >> 63) ? (key & ~(1ull << 63)) : ~key; }
// the bits of `key` above the digit of width `width` at `shift` (none on the first pass), and the digit
KDB_SELECT_HD inline uint64_t key_above(uint64_t key, int shift, int width) { return shift + width >= 64 ? 0 : key >> (shift + width); }
KDB_SELECT_HD inline uint32_t key_digit(uint64_t key, int shift, int width) { return (uint32_t)(key >> shift) & ((1u << width) - 1u); }

inline uint64_t key_of(double v) { uint64_t b; memcpy(&b, &v, 8); return key_of_bits(b); }
inline double value_of(uint64_t key) { const uint64_t b = bits_of_key(key); double v; memcpy(&v, &b, 8); return v; }

// histogram + rank -> the bucket that holds the element of that rank, and its rank inside the bucket.  false: fewer than rank + 1 elements.
inline bool narrow(const uint64_t *hist, int nbucket, uint64_t rank, uint32_t *digit, uint64_t *rest)
{
    uint64_t below = 0;
    for (int d = 0; d < nbucket; d++) {
        if (rank - below < hist[d]) { *digit = (uint32_t)d; *rest = rank - below; return true; }
        below += hist[d];
    }
    return false;
}

// One sample's select: the elements of ranks lo <= hi (hi is lo or lo + 1) among m.
struct Select {
    uint64_t prefix[2] = {0, 0};          // the key bits above the next digit, per target
    uint64_t rank[2] = {0, 0};            // the wanted rank among the elements under that prefix; with one target, both ranks are under prefix[0]
    int ntargets = 1;

    void start(uint64_t lo, uint64_t hi) { prefix[0] = prefix[1] = 0; rank[0] = lo; rank[1] = hi; ntargets = 1; }

    // hist0, hist1: the pass's histograms under prefix[0] and prefix[1] (hist1 is read only with two targets).  false: a rank has no element.
    bool step(const uint64_t *hist0, const uint64_t *hist1, int pass)
    {
        const int nbucket = 1 << pass_width(pass);
        uint32_t d0, d1;
        uint64_t r0, r1;
        if (!narrow(hist0, nbucket, rank[0], &d0, &r0)) return false;
        if (!narrow(ntargets == 2 ? hist1 : hist0, nbucket, rank[1], &d1, &r1)) return false;
        const uint64_t p0 = (prefix[0] << pass_width(pass)) | d0, p1 = (prefix[ntargets == 2 ? 1 : 0] << pass_width(pass)) | d1;
        prefix[0] = p0; prefix[1] = p1; rank[0] = r0; rank[1] = r1;
        if (p0 != p1) ntargets = 2;
        return true;
    }

    // after NPASS steps the prefixes are whole keys
    double low() const { return value_of(prefix[0]); }
    double high() const { return value_of(prefix[1]); }
};

// the median of m > 0 elements from its two middle order statistics: the middle one (m odd), or the arithmetic mean of the two (m even)
inline void median_ranks(uint64_t m, uint64_t *lo, uint64_t *hi) { *lo = (m - 1) / 2; *hi = m / 2; }
inline double median_of(double low, double high) { return (low + high) / 2; }

}  // namespace kdbselect
