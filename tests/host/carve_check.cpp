// carve_check.cpp - host check of sphx_carve.h, the one statement of a device buffer's layout from which the side
// families take both the bytes to allocate and every array's pointer.  Stand-alone: its own main, no GPU, no library.
//
// Random piece lists (1 .. 32 pieces; counts 0, 1, 3, 4, 5, 63, 64, 65, 1023; elements of 4, 8 and 64 bytes; natural or
// 16-byte alignment; some slack): every offset is the previous end rounded up to the piece's alignment, bytes() is the last
// end plus the slack, a piece of count 0 moves nothing, and - bound to a 16-byte-aligned block of exactly bytes() - every
// piece is written end to end with its own tag and read back intact (in bounds under ASan, no overlap).  A 33rd piece is
// refused.  Then the three padding rules the carver replaced, by their old formulas.  A carver that ignores the alignment
// argument must be caught.
#include "../../sph-code_amd/csrc/sphx_carve.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

struct Rec64 { double v[8]; };
static_assert(sizeof(Rec64) == 64 && alignof(Rec64) == 8, "a 64-byte record of doubles");

// the broken rule: the alignment argument is dropped
struct NoAlign : Carve {
    template <class T> void take(T*& p, size_t count, size_t = 0) { Carve::take(p, count); }
};

static size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static const size_t COUNTS[] = {0, 1, 3, 4, 5, 63, 64, 65, 1023};

struct Want { int kind; size_t count, size, align, off; };      // kind: 0 int, 1 double, 2 Rec64

template <class C> static long sweep_case(unsigned seed) {
    std::mt19937 rng(seed);
    const int np = 1 + (int)(rng() % 32);
    int* pi[32] = {nullptr};
    double* pd[32] = {nullptr};
    Rec64* pr[32] = {nullptr};
    Want w[32];
    C c;
    size_t end = 0, top = 0;
    for (int i = 0; i < np; ++i) {
        Want& q = w[i];
        q.kind = (int)(rng() % 3);
        q.count = COUNTS[rng() % 9];
        q.size = q.kind == 0 ? 4 : q.kind == 1 ? 8 : 64;
        const bool natural = rng() % 2 == 0;
        q.align = natural ? (q.kind == 0 ? alignof(int) : alignof(double)) : 16;
        if (q.kind == 0) { if (natural) c.take(pi[i], q.count); else c.take(pi[i], q.count, 16); }
        if (q.kind == 1) { if (natural) c.take(pd[i], q.count); else c.take(pd[i], q.count, 16); }
        if (q.kind == 2) { if (natural) c.take(pr[i], q.count); else c.take(pr[i], q.count, 16); }
        q.off = round_up(end, q.align);
        if (q.count > 0) end = q.off + q.count * q.size;        // (a piece of count 0 moves nothing)
        if (top < q.off) top = q.off;
        if (top < end) top = end;
    }
    static const size_t SLACKS[] = {0, 8, 16, 64};
    const size_t slack = SLACKS[rng() % 4];
    c.slack(slack);
    long bad = 0;
    bad += c.overflowed() || c.pieces() != np;
    for (int i = 0; i < np; ++i) bad += c.offset(i) != w[i].off;
    bad += c.bytes() != top + slack;
    if (c.bytes() == 0) return bad;
    void* block = nullptr;
    if (posix_memalign(&block, 16, c.bytes()) != 0) return bad + 1;
    c.bind(block);
    // every piece written end to end with its own tag (typed stores: UBSan sees a misaligned pointer), then all read back
    for (int i = 0; i < np; ++i) {
        const Want& q = w[i];
        char* at = q.kind == 0 ? (char*)pi[i] : q.kind == 1 ? (char*)pd[i] : (char*)pr[i];
        bad += at != (char*)block + c.offset(i);
        if ((size_t)(at - (char*)block) % q.align) { ++bad; continue; }       // (the broken rule: no store through it)
        for (size_t e = 0; e < q.count; ++e) {
            if (q.kind == 0) pi[i][e] = 0;
            if (q.kind == 1) pd[i][e] = 0.0;
            if (q.kind == 2) pr[i][e] = Rec64{};
        }
        std::memset(at, i + 1, q.count * q.size);
    }
    for (int i = 0; i < np; ++i) {
        const Want& q = w[i];
        const unsigned char* at = (const unsigned char*)block + c.offset(i);
        for (size_t b = 0; b < q.count * q.size; ++b)
            if (at[b] != (unsigned char)(i + 1)) { ++bad; break; }
    }
    std::free(block);
    return bad;
}

// a 33rd piece: an error state, nothing written, the 32 stand
static long overflow_case() {
    int* p[33] = {nullptr};
    Carve c;
    for (int i = 0; i < 32; ++i) c.take(p[i], 5);
    long bad = c.overflowed() || c.bytes() != 32 * 5 * sizeof(int);
    c.take(p[32], 5);
    bad += !c.overflowed() || c.pieces() != 32 || c.bytes() != 32 * 5 * sizeof(int);
    int block[32 * 5];
    c.bind(block);
    bad += p[31] != block + 31 * 5 || p[32] != nullptr;
    return bad;
}

// a piece of count 0 in the middle: the others where they were, its own pointer valid (inside bytes())
static long zero_case(size_t n) {
    int *a, *b, *z;
    double* d;
    Carve with, without;
    with.take(a, n + 1, 16); with.take(z, 0, 16); with.take(d, 0); with.take(b, n + 1);
    without.take(a, n + 1, 16); without.take(b, n + 1);
    long bad = with.offset(0) != without.offset(0) || with.offset(3) != without.offset(1) || with.bytes() < without.bytes();
    bad += with.offset(1) > with.bytes() || with.offset(2) > with.bytes() || with.offset(1) % 16 != 0;
    return bad;
}

// the old rules, by their formulas: the int blocks of the single-launch scan ((n + 4) & ~3 ints apart), the radiative
// phases' even counts of doubles ((c + 1) & ~1), and the sampler's flags (n + 1 used and four of head-room: (n + 8) & ~3)
template <class C> static long old_rules(size_t n) {
    long bad = 0;
    int *i0, *i1, *i2;
    C a;
    a.take(i0, n + 1, 16); a.take(i1, n + 1, 16); a.take(i2, n + 1, 16);
    const size_t n1 = (n + 4) & ~size_t(3);
    for (int q = 0; q < 3; ++q) bad += a.offset(q) != (size_t)q * n1 * sizeof(int);
    a.pad(16);
    bad += a.bytes() != 3 * n1 * sizeof(int);
    const size_t cs[] = {n, 3 * n, n + 1, 0, 5, 2 * n + 1};
    double* d[6];
    C b;
    size_t sum = 0;
    for (int q = 0; q < 6; ++q) {
        b.take(d[q], cs[q], 16);
        bad += b.offset(q) != sum * sizeof(double);
        sum += (cs[q] + 1) & ~size_t(1);
    }
    b.pad(16);
    bad += b.bytes() != sum * sizeof(double);
    int *wide, *woff;
    C f;
    f.take(wide, n + 5, 16); f.take(woff, n + 5, 16);
    bad += f.offset(1) != ((n + 8) & ~size_t(3)) * sizeof(int);
    return bad;
}

int main() {
    long bad = 0, broken = 0, cases = 0;
    for (unsigned seed = 1; seed <= 4000; ++seed, ++cases) {
        bad += sweep_case<Carve>(seed);
        broken += sweep_case<NoAlign>(seed) != 0;
    }
    bad += overflow_case(); ++cases;
    for (size_t n : {1, 2, 3, 4, 5, 63, 64, 65, 1023}) {
        bad += zero_case(n) + old_rules<Carve>(n);
        broken += old_rules<NoAlign>(n) != 0;
        cases += 2;
    }
    std::printf("sphx_carve: %ld violations in %ld cases\n", bad, cases);
    std::printf("broken rule: %ld cases wrong (must be > 0)\n", broken);
    return (bad == 0 && broken > 0) ? 0 : 1;
}
