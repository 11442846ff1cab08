// radphase_check.cpp - host replay of sphx_radphase_pair.h, the per-particle formulas of the radiative block
// (code_running.py:247-316 with nsc:976-1012) that the kernels of sphx_radphase.hip run.  Stand-alone: its own main, no
// GPU, no library.
//
// Seeded particles drive every regime of the bookkeeping: E_internal = 0 (the quotient is inf, nan_to_num makes it
// DBL_MAX), negative E_internal (the exp branch), NaN and zero lf2, T below t_cmb and above t_max, a cooling energy that
// underflows the exp, dust rows (the sixth root), stars (untouched but for the clamps); rows of s = 6 .. 32 species sit
// in exactly-sized allocations, so an index past a row is an error under the address sanitizer.  Every result is
// compared with the same formula evaluated in long double from the documentation in include/sphx.h, and held to the
// properties the block guarantees: clamped E and T inside their limits (or NaN), rows that sum to 1, fractions in
// [0, 0.99].  A rule that forgets nan_to_num must be caught.
#include "../../sph-code_amd/csrc/sphx_radphase_pair.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef long double ld;
static const double MUS[32] = {2.0158, 4.0026, 1.0079, 1.0074, 4.0021, 4.0016, 0.0005, 140.69, 60.08, 12.0107, 28.0855, 55.834, 100.39,
                               131.93, 40.096, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17};
static const double AMU = 1.66053906892e-27;

static ld ntn(ld v) {
    const double d = (double)v;
    if (d != d) return 0;
    if (d > DBL_MAX) return DBL_MAX;
    if (d < -DBL_MAX) return -DBL_MAX;
    return d;
}
// Tolerances, from the arithmetic and not from what the code gives (tests/radphase_oracle.py carries the same terms per
// element; this program cannot read it, so it uses their largest values over the regimes drawn here):
//   RT_SUM  1e-12: a quantity that is a ratio of sums over species (the project's bound for a sum evaluated in another
//           order or precision), mu, gamma, cross;
//   RT_EXP  4e-12: a quantity behind an exp or a root: the exponent x is itself a rounded quotient, and exp turns its
//           relative error of a few 2^-52 into |x| times that - |x| < 746 where the result is not 0, so 746 x 4 x 2^-52 =
//           6.6e-13 - plus 16 ulp for the function and RT_SUM for the gamma and mu inside; E_internal and T;
//   AT_FRAC 5e-16: 0.99 - 0.99 exp(-x) cancels for small x, so a destroyed fraction carries two roundings of 0.99 as an
//           ABSOLUTE error; a composition entry (at most 1) takes that from three fractions and its own sums: AT_ROW 2e-15.
static const double RT_SUM = 1e-12, RT_EXP = 4e-12, AT_FRAC = 5e-16, AT_ROW = 2e-15;
static bool close(double got, ld want, double rtol, double atol = 0.0) {
    const double w = (double)want;
    if (got != got || w != w) return got != got && w != w;
    if (got == w) return true;
    return std::fabs(got - w) <= rtol * std::fabs(w) + atol + 1e-300;
}
static ld coeff(ld x, bool broken) {
    if (!broken) x = ntn(x);
    return x >= 0 ? x + 1 : expl(x);
}

struct Particle { double pt, m, size, E, T, lf2, energy, mu_before, mom[3], vel[3]; std::vector<double> f; };

static Particle draw(std::mt19937& rng, int s, int regime) {
    std::uniform_real_distribution<double> u(0.0, 1.0);
    Particle p;
    p.f.resize(s);                                   // exactly s: a read past the row is out of bounds
    double tot = 0;
    for (int t = 0; t < s; ++t) { p.f[t] = u(rng) + (t < 3 ? 2.0 : 0.0); tot += p.f[t]; }
    for (int t = 0; t < s; ++t) p.f[t] /= tot;
    if (regime % 7 == 3) p.f[0] = 0.0;               // atoms_total = 0: the fraction is set to 0
    const double r = u(rng);
    p.pt = r < 0.2 ? 2.0 : (r < 0.25 ? 1.0 : 0.0);
    p.m = 1e30 * (1 + u(rng)); p.size = 1e14 * (1 + u(rng)); p.mu_before = 1 + u(rng);
    p.T = std::pow(10.0, -1 + 7 * u(rng));
    p.E = p.m / (1.67e-27 * p.mu_before) * 1.6 * 1.380649e-23 * std::pow(10.0, -1 + 7 * u(rng));
    p.lf2 = std::pow(10.0, 20 + 20 * u(rng));
    p.energy = std::pow(10.0, -30 + 12 * u(rng));
    switch (regime % 6) {
        case 1: p.E = 0.0; break;
        case 2: p.E = -p.E; break;
        case 3: p.lf2 = NAN; break;
        case 4: p.lf2 = 0.0; p.energy = 1e-8; break;
        case 5: p.energy = -p.energy; break;
        default: break;
    }
    for (int a = 0; a < 3; ++a) { p.mom[a] = 10 * (u(rng) - 0.5); p.vel[a] = 1e3 * (u(rng) - 0.5); }
    return p;
}

static long check(int s, unsigned seed, bool broken) {
    std::mt19937 rng(seed);
    long bad = 0;
    std::vector<double> gam(s), cs(s), fd(s);
    for (int t = 0; t < s; ++t) { gam[t] = t == 0 ? 1.4 : 5. / 3; cs[t] = t < 3 ? 7.875e-24 : 1e-62 + 1e-22 * (t > 6); fd[t] = t < 3 ? 0.3 + 0.2 * t : 0.0; }
    SphxRpConst c;
    c.t_cmb = 2.732; c.t_max = 1e4; c.k = 1.380649e-23; c.m_h = 1.0008 * AMU; c.sb = 5.670374419e-8; c.dt = 7.9e12; c.cooling_timescale = 2 * c.dt;
    for (int it = 0; it < 600; ++it) {
        Particle p = draw(rng, s, it);
        // ---- ionise + normalise ----
        std::vector<double> row(p.f);
        double frac[3] = {-1, -1, -1};
        const double ppj = 2.3e17;                    // photons per joule: the fractions span 0 .. 0.99
        if (p.pt != 1.0) sphx_rp_ionise_row(s, row.data(), p.m, p.lf2, ppj, fd.data(), MUS, cs.data(), AMU, frac);
        sphx_rp_normalise_row(s, row.data());
        ld smu = 0, scs = 0;
        for (int t = 0; t < s; ++t) { smu += (ld)p.f[t] * MUS[t] * AMU; scs += (ld)cs[t] * p.f[t]; }
        std::vector<ld> nf(p.f.begin(), p.f.end());
        if (p.pt != 1.0) {
            ld fr[3];
            for (int t = 0; t < 3; ++t) {
                const ld at = (ld)p.f[t] * ((ld)p.m / smu), ad = (ld)p.f[t] * cs[t] / scs * fd[t] * ((ld)ppj * p.lf2);
                fr[t] = ntn(0.99L - expl(-ntn(ad / at)) * 0.99L);
                if (at / AMU < 1e-10) fr[t] = 0;
                if (at / AMU < 0) fr[t] = 0.99;
                if (!close(frac[t], fr[t], RT_EXP, AT_FRAC) || !(frac[t] >= 0 && frac[t] <= 0.99)) ++bad;
            }
            nf[2] += (ld)p.f[0] * fr[0] * 2 - (ld)p.f[2] * fr[2]; nf[3] += (ld)p.f[2] * fr[2]; nf[4] += (ld)p.f[1] * fr[1];
            nf[5] += (ld)p.f[2] * fr[2] + (ld)p.f[1] * fr[1]; nf[0] -= (ld)p.f[0] * fr[0]; nf[1] -= (ld)p.f[1] * fr[1];
        }
        ld tot = 0, got_tot = 0;
        for (int t = 0; t < s; ++t) tot += nf[t];
        for (int t = 0; t < s; ++t) { if (!close(row[t], nf[t] / tot, RT_EXP, AT_ROW)) ++bad; got_tot += row[t]; }
        if (!(fabsl(got_tot - 1) < 1e-12)) ++bad;
        // ---- tables ----
        double mu, gamma, cross;
        sphx_rp_tables(s, row.data(), MUS, gam.data(), cs.data(), &mu, &gamma, &cross);
        ld a = 0, b = 0, d = 0, sf = 0;
        for (int t = 0; t < s; ++t) { a += (ld)row[t] * MUS[t]; b += (ld)row[t] * gam[t]; d += (ld)row[t] * cs[t]; sf += row[t]; }
        if (!close(mu, a / sf, RT_SUM) || !close(gamma, b / sf, RT_SUM) || !close(cross, d / sf, RT_SUM)) ++bad;
        // ---- heat ----
        double E = p.E, T = p.T;
        const int hit = sphx_rp_heat(c, p.pt, p.m, p.lf2, p.mu_before, mu, gamma, &E, &T);
        ld wE = p.E, wT = p.T;
        if (p.pt == 0.0) {
            wE = wE * coeff((ld)p.lf2 / p.E, broken);
            wT = wE / ((ld)p.m / ((ld)c.m_h * p.mu_before) * gamma * c.k);
        }
        const ld lo = (ld)c.t_cmb * ((ld)gamma * p.m * c.k) / ((ld)mu * c.m_h), hi = (ld)c.t_max * ((ld)gamma * p.m * c.k) / ((ld)mu * c.m_h);
        if (wE < lo) wE = lo;
        if (wE > hi) wE = hi;
        if (wT < c.t_cmb) wT = c.t_cmb;
        if (wT >= c.t_max) wT = c.t_max;
        if (!close(E, wE, RT_EXP) || !close(T, wT, RT_EXP)) ++bad;
        if (!(T != T || (T >= c.t_cmb && T <= c.t_max)) || !(E != E || (E >= (double)lo * (1 - 1e-12) && E <= (double)hi * (1 + 1e-12)))) ++bad;
        if ((hit & SPHX_RP_T_LO) && T != c.t_cmb) ++bad;
        if ((hit & SPHX_RP_T_HI) && T != c.t_max) ++bad;
        // ---- cool ----
        double E2 = E, T2 = T, v[3] = {p.vel[0], p.vel[1], p.vel[2]};
        sphx_rp_cool(c, p.pt, p.m, p.size, p.energy, p.lf2, p.mom, mu, gamma, cross, &E2, &T2, v);
        const ld npart = (ld)p.m / ((ld)c.m_h * mu);
        wE = E; wT = T;
        if (p.pt == 0.0) {
            ld c1 = coeff(-((ld)p.energy * npart) / E, broken) * expl(-(ld)c.dt / c.cooling_timescale * sqrtl((ld)T / 1e4));
            wE = wE * c1; wT = wE / (npart * gamma * c.k);
        } else if (p.pt == 2.0) {
            const ld h2 = (ld)p.size * p.size, optd = 1 - expl(-(npart * cross) * (9 / (4 * (ld)SPHX_RP_PI * h2)));
            wT = powl((ld)p.lf2 / (optd * 4 * SPHX_RP_PI * h2 * c.sb * 1e-5 * c.dt) + powl(c.t_cmb, 1.L / 6), 1.L / 6);
            wE = npart * c.k * wT * gamma;
        }
        if (wE < lo) wE = lo;
        if (wE > hi) wE = hi;
        if (wT < c.t_cmb) wT = c.t_cmb;
        if (wT >= c.t_max) wT = c.t_max;
        if (!close(E2, wE, RT_EXP) || !close(T2, wT, RT_EXP)) ++bad;
        for (int ax = 0; ax < 3; ++ax)
            if (v[ax] != (p.pt != 1.0 ? p.vel[ax] + p.mom[ax] : p.vel[ax])) ++bad;
    }
    return bad;
}

int main() {
    long bad = 0, broken = 0;
    unsigned seed = 77;
    for (int s : {6, 7, 15, 16, 32}) {
        bad += check(s, seed, false);
        broken += check(s, seed++, true);
    }
    std::printf("sphx_radphase_pair: %ld violations\n", bad);
    std::printf("broken rule: %ld violations\n", broken);
    return bad == 0 && broken > 0 ? 0 : 1;
}
