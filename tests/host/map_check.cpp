// map_check.cpp - host check of sphx_map_pair.h, the arithmetic and the tile walk of the projected maps (sphx_map.hip):
// the pipeline is replayed on the host - every particle's pixel span by sphx_map_span, its tile range, the tiles' lists
// in ascending id, each tile's list walked in batches of SPHX_MAP_BATCH through a staging array of exactly that size, one
// accumulator per pixel of the tile (the lanes beyond the image edge included) - and held against the plain statement:
// every pixel of the image adds the terms of ALL particles with s > 0 in ascending id.  The two must agree bit for bit,
// which is the claim that the bounding box on pixel centres never drops a pair with s > 0.  Also: sphx_map_span against a
// linear scan over the centres; the pixel centres do not decrease; and a deliberately broken rule (the box shrunk by one
// pixel) is seen to fail.  Stand-alone (own main), built by tests/test_map_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../sph-code_amd/csrc/sphx_map_pair.h"

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

struct Image { double cu, cv, wu, wv; int nu, nv; };
struct Part { SphxMapRec r; double R; };

static std::vector<Part> make_parts(std::mt19937_64& rng, int n, const Image& im, double rmin, double rmax) {
    std::uniform_real_distribution<double> u(-1.0, 1.0), rr(rmin, rmax), tt(-20.0, 200.0);
    std::vector<Part> p((size_t)n);
    for (Part& q : p) {
        q.R = rr(rng);
        q.r.xu = im.cu + 1.3 * im.wu * u(rng);
        q.r.xv = im.cv + 1.3 * im.wv * u(rng);
        q.r.R2 = q.R * q.R;
        q.r.c = sphx_map_coeff(1.0 + u(rng) * 0.5, q.R);
        q.r.T = tt(rng);
        q.r.gas = (rng() & 1) != 0 ? 1.0 : 0.0;
    }
    return p;
}

struct Pixel { double gc, dc, gt, dt; int cnt; };
static Pixel finish(const SphxMapAcc& a) {
    return Pixel{a.gc, a.dc, sphx_map_ratio(a.gn, a.gd), sphx_map_ratio(a.dn, a.dd), a.cnt};
}
static bool same_pixel(const Pixel& a, const Pixel& b) {
    return same_bits(a.gc, b.gc) && same_bits(a.dc, b.dc) && same_bits(a.gt, b.gt) && same_bits(a.dt, b.dt) && a.cnt == b.cnt;
}

// the plain statement
static std::vector<Pixel> brute(const std::vector<Part>& p, const Image& im, int want) {
    std::vector<Pixel> out((size_t)im.nu * (size_t)im.nv);
    for (int j = 0; j < im.nv; ++j)
        for (int i = 0; i < im.nu; ++i) {
            const double u = sphx_map_centre(im.cu, im.wu, im.nu, i), v = sphx_map_centre(im.cv, im.wv, im.nv, j);
            SphxMapAcc a;
            sphx_map_acc_zero(a);
            for (const Part& q : p) sphx_map_add(a, q.r, u, v, want);
            out[(size_t)j * (size_t)im.nu + (size_t)i] = finish(a);
        }
    return out;
}

// the kernels' route; shrink: the broken rule (the span cut by one pixel at each end)
static std::vector<Pixel> tiled(const std::vector<Part>& p, const Image& im, int want, int shrink, long long* pairs) {
    const int T = SPHX_MAP_TILE;
    const int ntx = (im.nu + T - 1) / T, nty = (im.nv + T - 1) / T;
    std::vector<std::vector<int>> list((size_t)ntx * (size_t)nty);
    *pairs = 0;
    for (size_t k = 0; k < p.size(); ++k) {                       // (ascending id: what the segmented sort restores)
        int ilo, ihi, jlo, jhi;
        sphx_map_span(im.cu, im.wu, im.nu, p[k].r.xu, p[k].R, &ilo, &ihi);
        sphx_map_span(im.cv, im.wv, im.nv, p[k].r.xv, p[k].R, &jlo, &jhi);
        ilo += shrink; ihi -= shrink; jlo += shrink; jhi -= shrink;
        if (ilo > ihi || jlo > jhi) continue;
        for (int ty = jlo / T; ty <= jhi / T; ++ty)
            for (int tx = ilo / T; tx <= ihi / T; ++tx) { list[(size_t)ty * (size_t)ntx + (size_t)tx].push_back((int)k); ++*pairs; }
    }
    std::vector<Pixel> out((size_t)im.nu * (size_t)im.nv);
    std::vector<SphxMapRec> stage((size_t)SPHX_MAP_BATCH);        // exactly the LDS array: a read beyond it is an error ASan sees
    for (int ty = 0; ty < nty; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            const std::vector<int>& L = list[(size_t)ty * (size_t)ntx + (size_t)tx];
            std::vector<SphxMapAcc> acc((size_t)(T * T));
            for (SphxMapAcc& a : acc) sphx_map_acc_zero(a);
            for (size_t base = 0; base < L.size(); base += SPHX_MAP_BATCH) {
                const size_t len = L.size() - base < (size_t)SPHX_MAP_BATCH ? L.size() - base : (size_t)SPHX_MAP_BATCH;
                for (size_t l = 0; l < len; ++l) stage[l] = p[(size_t)L[base + l]].r;
                for (int l = 0; l < T * T; ++l) {
                    const int i = tx * T + (l & (T - 1)), j = ty * T + l / T;
                    const double u = sphx_map_centre(im.cu, im.wu, im.nu, i), v = sphx_map_centre(im.cv, im.wv, im.nv, j);
                    for (size_t r = 0; r < len; ++r) sphx_map_add(acc[(size_t)l], stage[r], u, v, want);
                }
            }
            for (int l = 0; l < T * T; ++l) {
                const int i = tx * T + (l & (T - 1)), j = ty * T + l / T;
                if (i < im.nu && j < im.nv) out[(size_t)j * (size_t)im.nu + (size_t)i] = finish(acc[(size_t)l]);
            }
        }
    return out;
}

int main() {
    std::mt19937_64 rng(20240611u);
    long long violations = 0, checked = 0, broken = 0;
    const Image images[] = {{0.0, 0.0, 1.0, 1.0, 1, 1},     {0.3, -0.2, 1.0, 0.5, 15, 15}, {0.0, 0.0, 1.0, 1.0, 16, 16},
                            {1e3, -1e3, 2.0, 3.0, 17, 17},  {0.0, 0.0, 1.0, 1.0, 33, 65},  {-0.7, 0.1, 0.01, 0.02, 65, 33},
                            {1e17, 2e16, 9e16, 9e16, 40, 24}};
    const int want_all = SPHX_MAP_GAS_COLUMN | SPHX_MAP_DUST_COLUMN | SPHX_MAP_GAS_T | SPHX_MAP_DUST_T | SPHX_MAP_COUNT;
    for (const Image& im : images) {
        // the centres do not decrease, and the span is the linear scan's
        for (int i = 1; i < im.nu; ++i)
            if (sphx_map_centre(im.cu, im.wu, im.nu, i) < sphx_map_centre(im.cu, im.wu, im.nu, i - 1)) ++violations;
        for (const double scale : {0.02, 0.3, 4.0}) {
            const std::vector<Part> p = make_parts(rng, 700, im, 0.2 * scale * im.wu, scale * im.wu);
            for (const Part& q : p) {
                int lo, hi, slo = im.nu, shi = -1;
                sphx_map_span(im.cu, im.wu, im.nu, q.r.xu, q.R, &lo, &hi);
                for (int i = 0; i < im.nu; ++i)
                    if (std::fabs(sphx_map_centre(im.cu, im.wu, im.nu, i) - q.r.xu) <= q.R) { if (i < slo) slo = i; shi = i; }
                if (shi < 0) { if (lo <= hi) ++violations; }
                else if (lo != slo || hi != shi) ++violations;
                ++checked;
            }
            long long pairs = 0, pairs_b = 0;
            const std::vector<Pixel> ref = brute(p, im, want_all), got = tiled(p, im, want_all, 0, &pairs);
            for (size_t o = 0; o < ref.size(); ++o) { if (!same_pixel(ref[o], got[o])) ++violations; ++checked; }
            // an output left out leaves the others' bits alone
            const std::vector<Pixel> part = tiled(p, im, SPHX_MAP_DUST_COLUMN | SPHX_MAP_GAS_T, 0, &pairs_b);
            for (size_t o = 0; o < ref.size(); ++o)
                if (!same_bits(part[o].dc, ref[o].dc) || !same_bits(part[o].gt, ref[o].gt) || part[o].cnt != ref[o].cnt) ++violations;
            if (pairs != pairs_b) ++violations;
            const std::vector<Pixel> cut = tiled(p, im, want_all, 1, &pairs_b);
            for (size_t o = 0; o < ref.size(); ++o) if (!same_pixel(ref[o], cut[o])) ++broken;
        }
    }
    // the closed form: a particle right on a pixel centre gives c R^7 there
    {
        SphxMapRec r;
        r.xu = 0.25; r.xv = -0.5; r.R2 = 4.0; r.c = sphx_map_coeff(3.0, 2.0); r.T = 10.0; r.gas = 1.0;
        const double t = sphx_map_term(r.c, sphx_map_s(r, 0.25, -0.5));
        if (!same_bits(t, r.c * 128.0)) ++violations;
        if (sphx_map_s(r, 2.25, -0.5) != 0.0) ++violations;       // on the rim: s = 0 does not count
        SphxMapAcc a;
        sphx_map_acc_zero(a);
        sphx_map_add(a, r, 2.25, -0.5, want_all);
        if (a.cnt != 0) ++violations;
        ++checked;
    }
    std::printf("checked: %lld\n", checked);
    std::printf("broken rule: %lld pixels differ when the span is cut by a pixel\n", broken);
    std::printf("sphx_map: %lld violations\n", violations);
    return violations == 0 && broken > 0 ? 0 : 1;
}
