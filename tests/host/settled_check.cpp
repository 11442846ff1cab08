// settled_check.cpp - the rules of sphx_settled.h replayed on the host: which own values settle a row of pass 3, and
// that a quad's OR of "my partial sum is NaN" says exactly whether the row's total (p0 + p1) + (p2 + p3) is NaN.
// Built by tests/test_settled_cases_cpu.py, plain and with sanitizers.  Prints the number of violations, and the count
// of cases a deliberately wrong rule (infinite values taken as settled) gets wrong, to show that the check can fail.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../sph-code_amd/csrc/sphx_settled.h"

static double from_bits(uint64_t b) {
    double x;
    std::memcpy(&x, &b, sizeof x);
    return x;
}

int main() {
    long bad = 0, broken = 0, cases = 0;
    const double inf = std::numeric_limits<double>::infinity();
    // NaN of either sign and any payload, quiet and signalling
    std::vector<double> nans;
    const uint64_t payloads[] = {0x0008000000000000ull, 0x0000000000000001ull, 0x000FFFFFFFFFFFFFull, 0x0004000000000000ull,
                                 0x0000000012345678ull, 0x0007FFFFFFFFFFFFull};
    for (uint64_t p : payloads)
        for (uint64_t sign : {0ull, 0x8000000000000000ull}) nans.push_back(from_bits(sign | 0x7FF0000000000000ull | p));
    nans.push_back(std::nan(""));
    nans.push_back(-std::nan("1"));
    // everything else
    const std::vector<double> others = {inf, -inf, 0.0, -0.0, std::numeric_limits<double>::denorm_min(),
                                        -std::numeric_limits<double>::denorm_min(), from_bits(0x000FFFFFFFFFFFFFull),
                                        std::numeric_limits<double>::min(), std::numeric_limits<double>::max(),
                                        -std::numeric_limits<double>::max(), 1.0, -1.0, 3.5e-40, -7.25e33};
    for (double x : nans) {
        ++cases;
        if (!std::isnan(x)) { std::printf("test value is no NaN\n"); return 2; }
        if (!sphx_is_nan(x) || !sphx_row_settled(x, true, true)) ++bad;
        if (sphx_row_settled(x, false, true) || sphx_row_settled(x, true, false)) ++bad;   // no term at all / nothing to write
        // what the shortcut of pass 3 rests on: NaN times anything is NaN, zero and infinity included
        for (double y : others)
            if (!std::isnan(x * y) || !std::isnan(y * x) || !std::isnan((y + x * y) / 2.0)) ++bad;
    }
    for (double x : others) {
        ++cases;
        if (sphx_is_nan(x) || sphx_row_settled(x, true, true)) ++bad;
        const bool wrong_rule = !std::isfinite(x);                 // "not finite" in place of "NaN"
        if (wrong_rule != sphx_row_settled(x, true, true)) ++broken;
    }
    // the quad rule: all 16 NaN patterns of four partial sums, the others finite (several sets of values)
    const double fin[][4] = {{1.0, -2.0, 3.5, 0.25}, {0.0, -0.0, 0.0, 0.0}, {1e300, 1e300, -1e300, -1e300},
                             {4.9e-324, -4.9e-324, 1e-310, 0.0}, {-7.0, 7.0, -7.0, 7.0}};
    for (const auto& f : fin)
        for (int pat = 0; pat < 16; ++pat)
            for (double q : nans) {
                double p[4];
                bool s[4];
                for (int l = 0; l < 4; ++l) {
                    p[l] = ((pat >> l) & 1) ? q : f[l];
                    s[l] = sphx_is_nan(p[l]);
                }
                const double total = (p[0] + p[1]) + (p[2] + p[3]);
                ++cases;
                if (std::isnan(total) != sphx_quad_saturated(s[0], s[1], s[2], s[3])) ++bad;
                if (std::isnan(total) != (s[0] && s[1] && s[2] && s[3]) ) ++broken;     // AND in place of OR
                // a NaN partial stays NaN whatever is added afterwards
                for (int l = 0; l < 4; ++l)
                    if (s[l])
                        for (double y : others)
                            if (!std::isnan(p[l] + y)) ++bad;
            }
    // the wave rule on lane masks: every pattern in every row alone, then random waves with rows that do not sum
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int trial = 0; trial < 20000; ++trial) {
        uint64_t nan_mask, live;
        if (trial < 16 * 16) {                       // one row with the pattern, the others saturated or not live
            const int row = trial / 16, pat = trial % 16;
            nan_mask = ~0ull;
            nan_mask = (nan_mask & ~(0xFull << (4 * row))) | ((uint64_t)pat << (4 * row));
            live = (trial & 1) ? ~0ull : (0xFull << (4 * row));
        } else {
            nan_mask = next() & next();
            if (trial % 3 == 0) nan_mask |= next();
            live = 0;
            const uint64_t rows = next() | ((trial % 5 == 0) ? ~0ull : 0ull);
            for (int r = 0; r < 16; ++r)
                if ((rows >> r) & 1) live |= 0xFull << (4 * r);
            if (trial % 7 == 0) nan_mask |= live;   // every live row saturated
        }
        nan_mask &= live;                            // a lane that does not sum reports nothing (its ballot bit is 0)
        bool want = true;
        for (int r = 0; r < 16; ++r) {
            if (!((live >> (4 * r)) & 1)) continue;
            const unsigned q = (unsigned)(nan_mask >> (4 * r)) & 0xFu;
            want = want && sphx_quad_saturated(q & 1, (q >> 1) & 1, (q >> 2) & 1, (q >> 3) & 1);
        }
        ++cases;
        if (sphx_wave_saturated(nan_mask, live) != want) ++bad;
        if (sphx_wave_saturated(nan_mask, ~0ull) != want) ++broken;      // rows that do not sum taken as live
    }
    std::printf("sphx_settled: %ld violations in %ld cases\n", bad, cases);
    std::printf("broken rule: %ld cases wrong\n", broken);
    return bad == 0 ? 0 : 1;
}
