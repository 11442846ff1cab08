// Host replay of the fused cell count's run rule (tests/test_grid_runs_cpu.py builds and runs this).
//
// grid_count_fused (sphx_grid.hip) cuts each wave's 64 consecutive particles into runs of equal cell id; the first lane
// of a run adds the run's length to the cell's count with one atomic add, and every lane of the run takes the value
// that add returned plus its distance from the head as its arrival number (sphx_run_of_lane, sphx_runs.h).  Replayed
// here: clouds of cell ids cut into waves (the last one partial), the heads' atomic adds arriving in random order
// over all waves.  Checked for every cloud:
//   the histogram equals the plain count; the arrival numbers of every cell are a permutation of 0 .. count - 1; inside a
//   run they ascend with the lane; the number of atomic adds equals the number of runs.
// A rule that takes the wave's end, not the end of the active lanes, for the last run is replayed as well and must BREAK
// the histogram on partial waves - the evidence that this check can fail.
//
// usage: grid_runs_check [trials]      exit status 0: the rule holds in every trial and the broken rule was caught
#include "../../sph-code_amd/csrc/sphx_runs.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

SphxRun ignores_partial_waves(unsigned long long heads, int /*n_active*/, int lane) { return sphx_run_of_lane(heads, 64, lane); }

typedef SphxRun (*Rule)(unsigned long long, int, int);

struct Head { int wave, lane, len; };

// One launch over cell[0 .. n): returns the number of violations under `rule`; *atomics: how many adds it took
long replay(Rng& rng, const std::vector<int>& cell, int ncells, Rule rule, long* atomics, long* runs_expected) {
    const int n = (int)cell.size();
    const int nwaves = (n + 63) / 64;
    std::vector<unsigned long long> heads(nwaves, 0ull);
    std::vector<Head> adds;
    long bad = 0;
    for (int w = 0; w < nwaves; ++w) {
        const int n_active = n - 64 * w < 64 ? n - 64 * w : 64;
        for (int l = 0; l < n_active; ++l)                                  // (the kernel's ballot: active lanes only)
            if (l == 0 || cell[64 * w + l - 1] != cell[64 * w + l]) { heads[w] |= 1ull << l; ++*runs_expected; }
        for (int l = 0; l < n_active; ++l) {
            const SphxRun r = rule(heads[w], n_active, l);
            if (r.head == l) adds.push_back({w, l, r.len});
            if (r.head < 0 || r.head > l || !((heads[w] >> r.head) & 1ull)) { ++bad; continue; }
            if (cell[64 * w + r.head] != cell[64 * w + l]) ++bad;            // a lane belongs to its head's cell
        }
    }
    *atomics += (long)adds.size();
    for (size_t i = adds.size(); i > 1; --i) {                               // the order in which the atomic adds arrive
        const size_t j = (size_t)rng.below((int)i);
        const Head t = adds[i - 1]; adds[i - 1] = adds[j]; adds[j] = t;
    }
    std::vector<int> hist(ncells, 0), plain(ncells, 0), base(n, -1), rank(n, -1);
    for (const Head& h : adds) {
        const int c = cell[64 * h.wave + h.lane];
        base[64 * h.wave + h.lane] = hist[c];
        hist[c] += h.len;
    }
    for (int i = 0; i < n; ++i) {
        const int w = i / 64, l = i % 64;
        const int n_active = n - 64 * w < 64 ? n - 64 * w : 64;
        const SphxRun r = rule(heads[w], n_active, l);
        const int b = (r.head >= 0 && r.head <= l) ? base[64 * w + r.head] : -1;      // the broadcast from the head
        if (b < 0) { ++bad; continue; }
        rank[i] = b + (l - r.head);
        if (l > r.head && rank[i] != rank[i - 1] + 1) ++bad;                 // ascending inside a run
        ++plain[cell[i]];
    }
    for (int c = 0; c < ncells; ++c) if (hist[c] != plain[c]) ++bad;
    std::vector<std::vector<char>> seen(ncells);
    for (int c = 0; c < ncells; ++c) seen[c].assign((size_t)plain[c], 0);
    for (int i = 0; i < n; ++i) {
        const int c = cell[i], r = rank[i];
        if (r < 0 || r >= plain[c] || seen[c][r]) { ++bad; continue; }
        seen[c][r] = 1;
    }
    return bad;
}

// the clouds: kind 0 .. 6, n particles
std::vector<int> cloud(Rng& rng, int kind, int n, int* ncells) {
    std::vector<int> c(n);
    switch (kind) {
    case 0: *ncells = 1; for (int i = 0; i < n; ++i) c[i] = 0; break;                            // ONE cell: runs fill whole waves
    case 1: *ncells = n; for (int i = 0; i < n; ++i) c[i] = i; break;                            // every run of length 1
    case 2: *ncells = 2; for (int i = 0; i < n; ++i) c[i] = i & 1; break;                        // A B A B: equal, never adjacent
    case 3: *ncells = n; for (int i = 0; i < n; ++i) c[i] = i / 2; break;                        // pairs, some cut by a wave's end
    case 4: {                                                                                    // sorted, random run lengths
        int id = 0;
        for (int i = 0; i < n;) { const int len = 1 + rng.below(1 + rng.below(90)); for (int q = 0; q < len && i < n; ++q) c[i++] = id; ++id; }
        *ncells = id;
        break;
    }
    case 5: *ncells = 3; for (int i = 0; i < n; ++i) c[i] = rng.below(3); break;                 // a few cells, unsorted
    default: {                                                                                   // sorted runs whose ids come back later
        *ncells = 5;
        for (int i = 0; i < n;) { const int id = rng.below(5), len = 1 + rng.below(70); for (int q = 0; q < len && i < n; ++q) c[i++] = id; }
        break;
    }
    }
    return c;
}

}  // namespace

int main(int argc, char** argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 2000;
    Rng rng(20240611);
    long bad = 0, broken_bad = 0, atomics = 0, runs = 0, particles = 0, broken_atomics = 0, broken_runs = 0;
    const int fixed_n[] = {1, 2, 63, 64, 65, 127, 128, 129, 64 * 3 + 1, 300, 700, 1000};
    for (int t = 0; t < trials; ++t) {
        const int kind = t % 7;
        const int n = t < 7 * 12 ? fixed_n[t / 7] : 1 + rng.below(64 * 6);
        int ncells = 0;
        const std::vector<int> c = cloud(rng, kind, n, &ncells);
        particles += n;
        bad += replay(rng, c, ncells, sphx_run_of_lane, &atomics, &runs);
        if (n % 64) broken_bad += replay(rng, c, ncells, ignores_partial_waves, &broken_atomics, &broken_runs);
    }
    if (atomics != runs) { printf("atomic adds %ld != runs %ld\n", atomics, runs); ++bad; }
    printf("sphx_run_of_lane: %ld violations (%d clouds, %ld particles, %ld atomic adds)\n", bad, trials, particles, atomics);
    printf("broken rule: %ld violations\n", broken_bad);
    return (bad == 0 && broken_bad > 0) ? 0 : 1;
}
