// census_check.cpp - host check of sphx_census_terms.h, the term arithmetic and the LDS tile's places of the census
// kernel (sphx_census.hip): the kernel's tile loop is replayed on the host - every lane of a chunk lays its terms at
// sphx_cen_at(tq, j), lane q of a tile walks its quantity's rows left to right - and held against the plain statement:
// quantity q of the chunk is the left-to-right sum over the chunk's rows of term q.  Also: no two (quantity, row) pairs
// share a place and none lies outside the tile; the row sum equals an independent statement of NumPy's order; a row outside
// a quantity's mask gives +0.0 whatever it holds.  Stand-alone (own main), built by tests/test_census_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../sph-code_amd/csrc/sphx_census_terms.h"

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// NumPy's pairwise sum of a contiguous run of n < 128 values, stated on its own
static double np_sum(const std::vector<double>& v) {
    const size_t n = v.size();
    if (n < 8) {
        double res = 0.0;
        for (size_t i = 0; i < n; ++i) res += v[i];
        return res;
    }
    double r[8];
    for (int i = 0; i < 8; ++i) r[i] = v[(size_t)i];
    size_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int u = 0; u < 8; ++u) r[u] += v[i + (size_t)u];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += v[i];
    return res;
}

struct Chunk {
    int rows, s;
    std::vector<SphxCenRow> row;
    std::vector<double> f, mus;
};

static Chunk make_chunk(std::mt19937_64& rng, int rows, int s, bool poison) {
    std::uniform_real_distribution<double> u(0.1, 2.0);
    std::uniform_int_distribution<int> ty(0, 2);
    Chunk c;
    c.rows = rows; c.s = s;
    c.f.resize((size_t)rows * (size_t)(s > 0 ? s : 1));
    c.mus.resize((size_t)(s > 0 ? s : 1));
    for (double& m : c.mus) m = u(rng) * 10.0;
    for (double& x : c.f) x = u(rng);
    c.row.resize((size_t)rows);
    for (int j = 0; j < rows; ++j) {
        SphxCenRow& r = c.row[(size_t)j];
        r.m = u(rng) * 1e30; r.pt = (double)ty(rng);
        r.vx = u(rng) - 1.0; r.vy = u(rng) - 1.0; r.vz = u(rng) - 1.0;
        r.ax = u(rng) - 1.0; r.ay = u(rng) - 1.0; r.az = u(rng) - 1.0;
        r.E = u(rng) * 1e40;
        r.f = s > 0 ? &c.f[(size_t)j * (size_t)s] : nullptr;
        if (poison && r.pt == 2.0) {             // dust rows that must not reach a gas or star quantity
            if (j % 3 == 0) r.m = std::numeric_limits<double>::quiet_NaN();
            if (j % 3 == 1 && s > 0) c.f[(size_t)j * (size_t)s] = std::numeric_limits<double>::quiet_NaN();
            if (j % 3 == 2)
                for (int t = 0; t < s; ++t) c.f[(size_t)j * (size_t)s + (size_t)t] = 0.0;       // row sum 0
        }
        r.rowsum = s > 0 ? sphx_cen_row_sum(s, r.f, c.mus.data()) : 0.0;
    }
    return c;
}

// the kernel's tile loop; pitch_bug: the walk reads with a pitch of 256 (the broken rule)
static std::vector<double> replay(const Chunk& c, bool pitch_bug, long* violations) {
    const int nq = sphx_cen_nq(c.s);
    std::vector<double> part((size_t)nq, 0.0);
    std::vector<double> tile((size_t)SPHX_CEN_TILE * SPHX_CEN_PITCH);
    std::vector<char> taken(tile.size());
    for (int t = 0; t < sphx_cen_tiles(nq); ++t) {
        const int len = sphx_cen_tile_len(nq, t), q0 = t * SPHX_CEN_TILE;
        if (len < 1 || len > SPHX_CEN_TILE || q0 + len > nq) ++*violations;
        std::fill(taken.begin(), taken.end(), 0);
        for (int j = 0; j < SPHX_CEN_CHUNK; ++j) {
            const bool live = j < c.rows;
            for (int tq = 0; tq < len; ++tq) {
                const size_t at = sphx_cen_at(tq, j);
                if (at >= tile.size() || taken[at]) { ++*violations; continue; }
                taken[at] = 1;
                tile[at] = live ? sphx_cen_term(c.row[(size_t)j], q0 + tq, c.s, c.mus.data()) : 0.0;
            }
        }
        for (int j = 0; j < len; ++j) {
            double sum = 0.0;
            for (int row = 0; row < c.rows; ++row) sum += tile[pitch_bug ? (size_t)j * 256 + (size_t)row : sphx_cen_at(j, row)];
            part[(size_t)(q0 + j)] = sum;
        }
    }
    return part;
}

static long check_chunk(const Chunk& c, bool pitch_bug) {
    long bad = 0;
    const std::vector<double> part = replay(c, pitch_bug, &bad);
    const int nq = sphx_cen_nq(c.s);
    for (int q = 0; q < nq; ++q) {
        double sum = 0.0;
        for (int j = 0; j < c.rows; ++j) sum += sphx_cen_term(c.row[(size_t)j], q, c.s, c.mus.data());
        if (!same_bits(sum, part[(size_t)q]) && !(sum != sum && part[(size_t)q] != part[(size_t)q])) ++bad;
    }
    return bad;
}

int main() {
    std::mt19937_64 rng(20261021);
    long violations = 0, broken = 0;
    const int sizes[] = {0, 1, 7, 8, 15, 16, 32};
    const int rows[] = {1, 2, 255, 256};
    for (int s : sizes)
        for (int r : rows) {
            const Chunk c = make_chunk(rng, r, s, false);
            violations += check_chunk(c, false);
            broken += check_chunk(c, true);
            // the row sum against NumPy's order stated on its own
            for (int j = 0; j < r && s > 0; ++j) {
                std::vector<double> v((size_t)s);
                for (int t = 0; t < s; ++t) v[(size_t)t] = c.f[(size_t)j * (size_t)s + (size_t)t] * c.mus[(size_t)t];
                if (!same_bits(np_sum(v), c.row[(size_t)j].rowsum)) ++violations;
            }
            // the single terms against the driver's expressions
            for (int j = 0; j < r; ++j) {
                const SphxCenRow& w = c.row[(size_t)j];
                for (int ty = 0; ty < 3; ++ty) {
                    if (!same_bits(sphx_cen_term(w, ty, s, c.mus.data()), w.pt == (double)ty ? w.m : 0.0)) ++violations;
                    for (int t = 0; t < s; ++t) {
                        const double want = w.pt == (double)ty ? ((w.f[t] * c.mus[(size_t)t]) / w.rowsum) * w.m : 0.0;
                        if (!same_bits(sphx_cen_term(w, SPHX_CEN_FIXED + ty * s + t, s, c.mus.data()), want)) ++violations;
                    }
                }
                if (!same_bits(sphx_cen_term(w, SPHX_CEN_KIN2, s, c.mus.data()), w.m * ((w.vx * w.vx + w.vy * w.vy) + w.vz * w.vz))) ++violations;
                if (!same_bits(sphx_cen_term(w, SPHX_CEN_MA + 1, s, c.mus.data()), w.m * w.ay)) ++violations;
                if (!same_bits(sphx_cen_term(w, SPHX_CEN_MV + 2, s, c.mus.data()), w.m * w.vz)) ++violations;
            }
        }
    // masking: poisoned dust rows leave every gas and star quantity +0.0, bit for bit, and make a dust one NaN
    for (int s : {7, 15}) {
        const Chunk c = make_chunk(rng, 256, s, true);
        long nan_dust = 0;
        for (int j = 0; j < c.rows; ++j) {
            const SphxCenRow& w = c.row[(size_t)j];
            if (w.pt != 2.0) continue;
            const int gas_star[] = {SPHX_CEN_M_GAS, SPHX_CEN_M_STAR};
            for (int q : gas_star)
                if (!same_bits(sphx_cen_term(w, q, s, c.mus.data()), 0.0)) ++violations;
            for (int q = SPHX_CEN_FIXED; q < SPHX_CEN_FIXED + 2 * s; ++q)
                if (!same_bits(sphx_cen_term(w, q, s, c.mus.data()), 0.0)) ++violations;
            for (int q = SPHX_CEN_FIXED + 2 * s; q < SPHX_CEN_FIXED + 3 * s; ++q) {
                const double v = sphx_cen_term(w, q, s, c.mus.data());
                if (v != v) ++nan_dust;
            }
        }
        if (nan_dust == 0) ++violations;
        violations += check_chunk(c, false);
    }
    std::printf("sphx_census: %ld violations\n", violations);
    std::printf("broken rule: %ld chunks' sums differ under a walk with pitch 256\n", broken);
    return violations == 0 ? 0 : 1;
}
