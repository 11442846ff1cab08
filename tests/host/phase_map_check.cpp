// phase_map_check.cpp - host replay of sphx_phase_map.h, the slot arithmetic that turns the step's own neighbour list
// (K-major, one column per processing position, entries storage slots) into the list in caller ids that
// sphx_state_dust_phase and sphx_state_download_neighbors use.  Stand-alone: its own main, no GPU, no library.
//
// For random storage orders (id), processing orders (qorder, or none) and lists with missing entries it runs the two
// passes lane by lane as the kernels do and compares every entry with a direct construction from the particles' own
// lists in caller ids; then the (n,k) int64 form.  A rule that forgets the processing order must be caught.
#include "../../sph-code_amd/csrc/sphx_phase_map.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

static long check(int n, int k, bool with_qorder, unsigned seed, bool broken) {
    std::mt19937 rng(seed);
    const int npad = (n + 63) & ~63;
    // truth: caller id i has the list L[i][kk] in caller ids, -1 = missing (a suffix of the row, as a short search leaves it)
    std::vector<int> L((size_t)n * k);
    for (int i = 0; i < n; ++i) {
        const int have = std::min(k, n);
        for (int kk = 0; kk < k; ++kk) L[(size_t)i * k + kk] = kk == 0 ? i : (kk < have ? (int)(rng() % (unsigned)n) : -1);
    }
    std::vector<int> id(n), slot_of(n), qorder(n), col_of_slot(n);
    std::iota(id.begin(), id.end(), 0);
    std::shuffle(id.begin(), id.end(), rng);
    for (int j = 0; j < n; ++j) slot_of[id[j]] = j;
    std::iota(qorder.begin(), qorder.end(), 0);
    if (with_qorder) std::shuffle(qorder.begin(), qorder.end(), rng);
    for (int p = 0; p < n; ++p) col_of_slot[qorder[p]] = p;
    // the step's list: column p = the particle in slot qorder[p], entries storage slots; pad columns hold garbage
    std::vector<int> nbr((size_t)k * npad, 0x7fffffff);
    for (int p = 0; p < n; ++p) {
        const int i = id[qorder[p]];
        for (int kk = 0; kk < k; ++kk) {
            const int v = L[(size_t)i * k + kk];
            nbr[sphx_phase_at(kk, npad, p)] = v < 0 ? -1 : slot_of[v];
        }
    }
    const int* qo = with_qorder ? qorder.data() : nullptr;
    std::vector<int> col(n, -7), out((size_t)k * npad, -7);
    for (int p = 0; p < n; ++p) sphx_phase_col_lane(broken ? nullptr : qo, id.data(), p, col.data());
    for (long long e = 0; e < (long long)k * npad; ++e) {
        const int kk = (int)(e / npad), i = (int)(e - (long long)kk * npad);
        out[(size_t)e] = sphx_phase_entry(nbr.data(), id.data(), col.data(), n, npad, kk, i);
    }
    long bad = 0;
    for (int kk = 0; kk < k; ++kk)
        for (int i = 0; i < npad; ++i) {
            const int want = i < n ? L[(size_t)i * k + kk] : -1;
            bad += out[sphx_phase_at(kk, npad, i)] != want;
        }
    for (long long e = 0; e < (long long)n * k; ++e) {
        const int v = L[(size_t)e];
        bad += sphx_phase_entry64(out.data(), n, npad, k, e) != (v < 0 ? (long long)n : (long long)v);
    }
    return bad;
}

int main() {
    const int ns[] = {1, 2, 33, 63, 64, 65, 257, 2049}, ks[] = {1, 7, 40, 64};
    long bad = 0, broken = 0;
    unsigned seed = 1;
    for (int n : ns)
        for (int k : ks)
            for (int q = 0; q < 2; ++q) {
                bad += check(n, k, q == 1, seed, false);
                if (q == 1 && n > 2) broken += check(n, k, true, seed, true);
                ++seed;
            }
    std::printf("sphx_phase_map: %ld violations\n", bad);
    std::printf("broken rule: %ld violations (must be > 0)\n", broken);
    return (bad == 0 && broken > 0) ? 0 : 1;
}
