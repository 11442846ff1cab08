// revlist_check.cpp - the two size rules of sphx_revlist.h checked on the host by brute force: the bits the segmented
// sort of a reverse list looks at, and where the sorted half lies behind the raw one.  Built by tests/test_phase_cpu.py,
// plain and with sanitizers.  Prints the number of violations, and the count of cases two deliberately wrong rules (the
// bits of key_end - 1's width without the floor of one; the sorted half M ints behind the raw one) get wrong, to show
// that the check can fail.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sph-code_amd/csrc/sphx_revlist.h"

int main() {
    long bad = 0, broken = 0, cases = 0;
    // bits(key_end): the least b in [1, 32] with 2^b >= key_end
    const unsigned long long ends[] = {1, 2, 3, 4, 5, (1ull << 16) - 1, 1ull << 16, (1ull << 16) + 1, (1ull << 31) - 16};
    for (unsigned long long key_end : ends) {
        unsigned want = 0;
        for (unsigned b = 1; b <= 32 && !want; ++b)
            if ((1ull << b) >= key_end) want = b;
        if (!want) { std::printf("no b for key_end %llu\n", key_end); return 2; }
        ++cases;
        if (sphx_rev_bits(key_end) != want) ++bad;
        unsigned width = 0;                                  // the wrong rule: bits needed to write key_end itself, no floor
        while ((1ull << width) < key_end) ++width;
        if (width != want) ++broken;
        // every key below key_end survives the sort's mask
        const unsigned long long mask = (1ull << sphx_rev_bits(key_end)) - 1;
        if (((key_end - 1) & mask) != key_end - 1) ++bad;
    }
    // the layout: raw [0, M), sorted [at, at + M), both inside the ints the builder ensures; really written and read here
    for (size_t M : {size_t(0), size_t(1), size_t(3), size_t(4), size_t(5), size_t(1023)}) {
        const size_t at = sphx_rev_sorted_at(M), ints = sphx_rev_ints(M);
        ++cases;
        if (at < M || (at * sizeof(int)) % 16 != 0 || at + M > ints) ++bad;
        if ((M * sizeof(int)) % 16 != 0) ++broken;            // the wrong rule: the sorted half at M
        std::vector<int> buf(ints, -1);
        int *raw = buf.data(), *sorted = buf.data() + at;
        for (size_t u = 0; u < M; ++u) raw[u] = (int)(M - u);
        for (size_t u = 0; u < M; ++u) sorted[u] = (int)(u + 1);
        for (size_t u = 0; u < M; ++u)
            if (raw[u] != (int)(M - u)) ++bad;                // the halves do not overlap
    }
    std::printf("sphx_revlist: %ld violations in %ld cases\n", bad, cases);
    std::printf("broken rule: %ld cases wrong\n", broken);
    return bad == 0 ? 0 : 1;
}
