// update_rows_check.cpp - a check of sphx_update_loads_visc (sphx_update_rows.h) on the host, and of nothing more: on
// random byte arrays a row takes pass 3's outputs as NaN exactly when its byte is not 0 (any non-zero byte is "settled",
// not only 1), and a launch without bytes loads for every row.  The update is one launch and a row is in one class by
// construction, so there is no partition of two launches to test; that dt is written by thread 0 whatever row 0's byte
// is follows from sphx_update_writes_dt not taking the byte, and is replayed only to pin that signature.
// Built by tests/test_update_rows_cpu.py, plain and with sanitizers.  Prints the number of violations, and the count of
// cases a deliberately wrong rule (only the byte 1 taken as settled) gets wrong, to show that the check can fail.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sph-code_amd/csrc/sphx_update_rows.h"

// what integrate_kernel does with the rules, thread by thread: who writes dt, who loads va / vh
struct Launch { std::vector<int> loads, constants; int dt_writes = 0; };
static Launch replay(const std::vector<unsigned char>* bytes, int n) {
    Launch l;
    l.loads.assign((size_t)n, 0);
    l.constants.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        if (sphx_update_writes_dt(i)) ++l.dt_writes;
        if (sphx_update_loads_visc(bytes != nullptr, bytes ? (*bytes)[(size_t)i] : 0)) ++l.loads[i];
        else ++l.constants[i];
    }
    return l;
}
// the wrong rule: a byte is "settled" only when it is exactly 1
static bool wrong_loads_visc(bool by_byte, unsigned char b) { return !by_byte || b != 1; }

int main() {
    long bad = 0, broken = 0, cases = 0;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int trial = 0; trial < 4000; ++trial) {
        // sizes around the launch's block of 256, and the classes' extremes: none settled, all settled, few of either
        const int sizes[] = {1, 2, 63, 64, 255, 256, 257, 500, 512, 1536, 4099};
        const int n = sizes[trial % 11];
        std::vector<unsigned char> bytes((size_t)n);
        const int kind = (trial / 11) % 6;
        for (int i = 0; i < n; ++i) {
            const uint64_t r = next();
            switch (kind) {
                case 0: bytes[i] = 0; break;
                case 1: bytes[i] = 1; break;
                case 2: bytes[i] = (unsigned char)(r & 1); break;
                case 3: bytes[i] = (unsigned char)((r % 16) == 0); break;
                case 4: bytes[i] = (unsigned char)((r % 16) != 0); break;
                default: bytes[i] = (unsigned char)((r & 1) ? (1 + (r >> 8) % 255) : 0); break;    // any non-zero byte
            }
        }
        if (kind == 3 || kind == 4) bytes[0] = (unsigned char)(trial & 1);       // row 0 of either class
        const Launch plain = replay(nullptr, n), by_byte = replay(&bytes, n);
        ++cases;
        bool wrong = false;
        for (int i = 0; i < n; ++i) {
            if (plain.loads[i] != 1 || plain.constants[i] != 0) ++bad;                        // no bytes: every row loads
            if (by_byte.constants[i] != (bytes[i] != 0 ? 1 : 0)) ++bad;                       // the class by the byte alone
            wrong = wrong || wrong_loads_visc(true, bytes[i]) != (bytes[i] == 0);
        }
        if (wrong) ++broken;
        // dt: thread 0's, with row 0 of either class (the function does not see the byte)
        if (plain.dt_writes != 1 || by_byte.dt_writes != 1) ++bad;
    }
    std::printf("sphx_update_rows: %ld violations in %ld cases\n", bad, cases);
    std::printf("broken rule: %ld cases wrong\n", broken);
    return bad == 0 ? 0 : 1;
}
