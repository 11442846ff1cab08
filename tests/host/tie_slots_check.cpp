// Host replay of the grouped search's tie-list reservations (tests/test_tie_clouds_cpu.py builds and runs this).
//
// In the kernel each of a query's four lanes reserves room for its entries with one atomic add on the list's count, the
// four lanes then vote (any reservation that crosses the capacity fails the whole query over), and every lane writes what
// kg_tie_slots (sphx_knn_group.h) tells it to.  The tie blocks of the launch that follows walk min(count, cap) slots.
// Invariant checked here, over random interleavings of the lanes' atomic adds around the capacity:
//   every slot below min(count, cap) is written exactly once; a real entry only by a certified query; nothing at or
//   beyond cap.
// The rule the kernel had before (a query that failed the vote writes nothing) is replayed as well and must BREAK the
// invariant - the evidence that this check can fail.
//
// usage: tie_slots_check [trials]      exit status 0: the rule holds in every trial and the former rule broke it
#define SPHX_KG_TIE_SLOTS_ONLY
#include "../../sph-code_amd/csrc/sphx_knn_group.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

// the former rule: only a query still certified after the vote writes (all of its slots; it never crossed cap)
KgTieSlots former_tie_slots(int /*base*/, int ne, int /*cap*/, bool certified) {
    KgTieSlots s;
    s.nwrite = certified ? ne : 0;
    s.real = true;
    return s;
}

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct Lane { int quad, ne, base; };

typedef KgTieSlots (*Rule)(int, int, int, bool);

// One search: `nquads` queries of four lanes, lane l of a quad reserving ne entries (drawn by `draw`), the atomic adds
// in random order.  Returns the number of invariant violations under `rule`.
template <class Draw>
long replay(Rng& rng, int cap, int nquads, Draw draw, Rule rule, int* crossed_exactly) {
    std::vector<Lane> lanes;
    for (int q = 0; q < nquads; ++q)
        for (int l = 0; l < 4; ++l) {
            const int ne = draw(rng, q, l);
            if (ne > 0) lanes.push_back({q, ne, 0});
        }
    for (size_t i = lanes.size(); i > 1; --i) {             // the order in which the atomic adds arrive
        const size_t j = (size_t)rng.below((int)i);
        const Lane t = lanes[i - 1]; lanes[i - 1] = lanes[j]; lanes[j] = t;
    }
    long long count = 0;
    std::vector<char> over(nquads, 0);
    for (Lane& L : lanes) {
        L.base = (int)count;
        count += L.ne;
        if (count == cap && crossed_exactly) ++*crossed_exactly;      // a reservation that ends exactly on the capacity
        if (kg_tie_overflows(L.base, L.ne, cap)) over[L.quad] = 1;   // (the vote: any lane of the quad)
    }
    // the list, with room beyond cap so that a write there is seen rather than a fault
    const long long span = count > cap ? count : cap;
    std::vector<int> writes((size_t)span + 16, 0), reals((size_t)span + 16, 0), bad_real((size_t)span + 16, 0);
    for (const Lane& L : lanes) {
        const bool certified = !over[L.quad];
        const KgTieSlots ts = rule(L.base, L.ne, cap, certified);
        for (int j = 0; j < L.ne; ++j) {
            if (j >= ts.nwrite) continue;
            const size_t slot = (size_t)L.base + (size_t)j;
            ++writes[slot];
            if (ts.real) { ++reals[slot]; if (!certified) ++bad_real[slot]; }
        }
    }
    long bad = 0;
    const long long walked = count < cap ? count : cap;
    for (long long s = 0; s < (long long)writes.size(); ++s) {
        if (s < walked) { if (writes[(size_t)s] != 1) ++bad; }
        else if (s >= cap) { if (writes[(size_t)s] != 0) ++bad; }
        if (bad_real[(size_t)s]) ++bad;
    }
    // a certified query's entries are all there and real
    for (const Lane& L : lanes)
        if (!over[L.quad])
            for (int j = 0; j < L.ne; ++j)
                if (reals[(size_t)L.base + (size_t)j] != 1) ++bad;
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 4000;
    long bad_new = 0, bad_former = 0, trials_former_broke = 0;
    int exact = 0, runs = 0;
    Rule rules[2] = {kg_tie_slots, former_tie_slots};
    for (int t = 0; t < trials; ++t) {
        for (int which = 0; which < 2; ++which) {
            Rng rng((uint64_t)t + 1);                         // both rules see the same searches
            const int cap = 8 + rng.below(120);
            long bad = 0;
            // (a) one entry per lane, about 0.5 .. 2 x cap entries in all
            {
                const int nquads = cap / 8 + 1 + rng.below(cap / 2 + 1);
                bad += replay(rng, cap, nquads, [](Rng&, int, int) { return 1; }, rules[which], &exact);
            }
            // (b) up to eight per lane, some lanes none
            {
                const int nquads = 1 + rng.below(cap / 4 + 2);
                bad += replay(rng, cap, nquads, [](Rng& r, int, int) { return r.below(9); }, rules[which], &exact);
            }
            // (c) a crossing that lands exactly on the capacity: cap entries by single lanes, then more
            {
                // lanes whose sizes sum to exactly cap arrive first (in any order), the lanes of a few more queries after them
                const int extra = 1 + rng.below(6);
                std::vector<int> sizes;
                int left = cap;
                while (left > 0) { int ne = 1 + rng.below(8); if (ne > left) ne = left; sizes.push_back(ne); left -= ne; }
                const int nlead = (int)sizes.size();
                // replay by hand: leading lanes in random order, then the extra quads' lanes
                Rng r2(rng.next());
                std::vector<Lane> lanes;
                for (int i = 0; i < nlead; ++i) lanes.push_back({i / 4, sizes[(size_t)i], 0});
                for (size_t i = lanes.size(); i > 1; --i) {
                    const size_t j = (size_t)r2.below((int)i);
                    const Lane tt = lanes[i - 1]; lanes[i - 1] = lanes[j]; lanes[j] = tt;
                }
                const int q0 = (nlead + 3) / 4;
                for (int q = 0; q < extra; ++q)
                    for (int l = 0; l < 4; ++l) { const int ne = r2.below(4); if (ne) lanes.push_back({q0 + q, ne, 0}); }
                const int nquads = q0 + extra;
                long long count = 0;
                std::vector<char> over((size_t)nquads, 0);
                bool landed = false;
                for (Lane& L : lanes) {
                    L.base = (int)count; count += L.ne;
                    if (count == cap) landed = true;
                    if (kg_tie_overflows(L.base, L.ne, cap)) over[(size_t)L.quad] = 1;
                }
                if (!landed) { fprintf(stderr, "scenario (c) did not land on the capacity\n"); return 2; }
                ++exact;
                std::vector<int> writes((size_t)count + 16, 0);
                for (const Lane& L : lanes) {
                    const bool certified = !over[(size_t)L.quad];
                    const KgTieSlots ts = rules[which](L.base, L.ne, cap, certified);
                    for (int j = 0; j < L.ne && j < ts.nwrite; ++j) {
                        ++writes[(size_t)L.base + (size_t)j];
                        if (ts.real && !certified) ++bad;
                    }
                    // the lanes that filled the list exactly are certified and complete
                    if (L.quad < q0 && (over[(size_t)L.quad] || ts.nwrite != L.ne || !ts.real)) ++bad;
                }
                for (long long s = 0; s < (long long)writes.size(); ++s)
                    if (writes[(size_t)s] != (s < cap ? 1 : 0)) ++bad;
            }
            if (which == 0) { bad_new += bad; ++runs; }
            else { bad_former += bad; if (bad) ++trials_former_broke; }
        }
    }
    printf("trials %d, reservations ending exactly on the capacity %d\n", runs, exact);
    printf("kg_tie_slots: %ld violations\n", bad_new);
    printf("former rule:  %ld violations in %ld trials\n", bad_former, trials_former_broke);
    if (bad_new != 0) { printf("FAIL: the rule breaks the invariant\n"); return 1; }
    if (trials_former_broke == 0) { printf("FAIL: the former rule never broke the invariant - the check has no teeth\n"); return 1; }
    if (exact == 0) { printf("FAIL: no reservation ended exactly on the capacity\n"); return 1; }
    printf("OK\n");
    return 0;
}
