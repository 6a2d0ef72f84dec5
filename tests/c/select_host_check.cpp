// The host side of kdb_size_factors' radix select (kmerdb_amd/csrc/kdb_select_host.cpp.h) alone, for AddressSanitizer + UBSan on the CPU:
// the key transform and the narrowing step, run as a complete host radix select over arrays of doubles -- the histograms the device would
// make are made here with the same key functions -- against a sort.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o select_host_check tests/c/select_host_check.cpp && ./select_host_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../kmerdb_amd/csrc/kdb_select_host.cpp.h"

static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); bad++; } } while (0)

static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

// what select_kernel does in one pass, for one sample; exactly sized histograms: a digit out of range is the sanitizer's to find
static void histograms(const std::vector<double> &v, const kdbselect::Select &s, int pass, std::vector<uint64_t> &h0, std::vector<uint64_t> &h1)
{
    const int shift = kdbselect::pass_shift(pass), width = kdbselect::pass_width(pass);
    h0.assign((size_t)1 << width, 0);
    h1.assign((size_t)1 << width, 0);
    for (double x : v) {
        const uint64_t key = kdbselect::key_of(x), above = kdbselect::key_above(key, shift, width);
        const uint32_t d = kdbselect::key_digit(key, shift, width);
        if (above == s.prefix[0]) h0[d]++;
        if (s.ntargets == 2 && above == s.prefix[1]) h1[d]++;
    }
}

// -> the pass at which the two ranks parted (NPASS if they never did)
static int check_median(const std::vector<double> &v)
{
    std::vector<double> sorted(v);
    std::sort(sorted.begin(), sorted.end(), [](double a, double b) { return kdbselect::key_of(a) < kdbselect::key_of(b); });
    for (size_t i = 1; i < sorted.size(); i++) CHECK(sorted[i - 1] <= sorted[i]);                    // the key orders like the value
    const uint64_t m = v.size();
    uint64_t lo, hi;
    kdbselect::median_ranks(m, &lo, &hi);
    CHECK(lo == (m - 1) / 2 && hi == m / 2 && hi - lo == (m % 2 == 0 ? 1u : 0u));
    kdbselect::Select s;
    s.start(lo, hi);
    int parted = kdbselect::NPASS;
    std::vector<uint64_t> h0, h1;
    for (int pass = 0; pass < kdbselect::NPASS; pass++) {
        histograms(v, s, pass, h0, h1);
        CHECK(s.step(h0.data(), h1.data(), pass));
        if (s.ntargets == 2 && parted == kdbselect::NPASS) parted = pass;
    }
    CHECK(bits(s.low()) == bits(sorted[lo]) && bits(s.high()) == bits(sorted[hi]));
    std::vector<double> nth(v);
    std::nth_element(nth.begin(), nth.begin() + hi, nth.end());
    CHECK(s.high() == nth[hi]);
    CHECK(kdbselect::median_of(s.low(), s.high()) == (sorted[lo] + sorted[hi]) / 2);
    return parted;
}

static double from_bits(uint64_t b) { double v; memcpy(&v, &b, 8); return v; }

int main()
{
    // the digits cover the key exactly once, top down
    int covered = 0;
    for (int p = 0; p < kdbselect::NPASS; p++) {
        CHECK(kdbselect::pass_shift(p) + kdbselect::pass_width(p) == 64 - covered);
        covered += kdbselect::pass_width(p);
    }
    CHECK(covered == 64 && kdbselect::pass_shift(kdbselect::NPASS - 1) == 0);
    // the key transform and its inverse
    for (double v : {0.0, -0.0, 1.0, -1.0, 1e-300, -1e-300, 5e-324, -5e-324, 1e300, -1e300, (double)INFINITY, -(double)INFINITY})
        CHECK(bits(kdbselect::value_of(kdbselect::key_of(v))) == bits(v));
    CHECK(kdbselect::key_of(-0.0) + 1 == kdbselect::key_of(0.0));
    CHECK(kdbselect::key_of(-1.0) < kdbselect::key_of(-0.5) && kdbselect::key_of(-0.5) < kdbselect::key_of(-0.0) && kdbselect::key_of(0.0) < kdbselect::key_of(0.5));

    // m = 1, 2, 3
    check_median({0.25});
    check_median({-3.5});
    check_median({1.0, 2.0});
    check_median({2.0, -2.0});
    check_median({3.0, 1.0, 2.0});
    check_median({-1.0, -1.0, 5.0});
    // all equal, odd and even
    check_median(std::vector<double>(7, 0.125));
    check_median(std::vector<double>(8, -0.125));
    // negatives, positives and both zeros; the two middle ranks are -0.0 and +0.0
    CHECK(check_median({-2.0, -1.0, -0.0, 0.0, 1.0, 2.0}) == 0);                            // -0.0 and +0.0 differ in the key's top bit
    check_median({-0.0, -0.0, 0.0, 0.0, 0.0});
    check_median({0.0, -0.0});
    // values that differ only in the lowest digit (the last 9 bits)
    {
        std::vector<double> v;
        for (uint64_t i = 0; i < 300; i++) v.push_back(from_bits(bits(1.5) + (i * 7) % 512));
        check_median(v);
        v.push_back(from_bits(bits(1.5) + 511));
        check_median(v);
    }
    // even m: the two middle ranks part at the first, a middle and the last digit
    CHECK(check_median({-1.0, -0.5, 0.5, 1.0}) == 0);                                          // the sign
    CHECK(check_median({1.0, from_bits(bits(1.0) + (1ull << 25)), 0.5, 4.0}) == 3);            // bit 25 is in the digit at shift 20
    CHECK(check_median({1.0, from_bits(bits(1.0) + 1), 0.5, 4.0}) == kdbselect::NPASS - 1);    // the last bit
    CHECK(check_median({1.0, 1.0, 0.5, 4.0}) == kdbselect::NPASS);                             // never: the two are equal
    // a few hundred, many ties, both signs; every size from 200 on for a while: odd and even
    std::mt19937_64 rng(11);
    for (int round = 0; round < 24; round++) {
        std::vector<double> v(200 + round);
        for (auto &x : v) {
            const uint64_t r = rng();
            x = (r % 3 == 0) ? ((double)((r >> 8) % 9) - 4.0) * 0.34657359027997264 : std::ldexp((double)(r >> 11), -50) - 3.0;
        }
        check_median(v);
    }
    // a rank with no element is refused, not answered
    {
        std::vector<uint64_t> h(kdbselect::NBUCKET, 0);
        h[5] = 2;
        uint32_t d;
        uint64_t rest;
        CHECK(kdbselect::narrow(h.data(), kdbselect::NBUCKET, 1, &d, &rest) && d == 5 && rest == 1);
        CHECK(!kdbselect::narrow(h.data(), kdbselect::NBUCKET, 2, &d, &rest));
        kdbselect::Select s;
        s.start(2, 3);
        CHECK(!s.step(h.data(), h.data(), 0));
    }
    if (bad) { printf("%d check(s) failed\n", bad); return 1; }
    printf("select host check ok\n");
    return 0;
}
