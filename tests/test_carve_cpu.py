"""CPU test of sphx_carve.h (no GPU): the side families state each device buffer's layout once, as a list of pieces, and take
both the bytes to allocate and every array's pointer from it.  tests/host/carve_check.cpp checks the offset rule, the total,
zero counts, the capacity and - under ASan / UBSan - that the pieces of a block of exactly that size neither overlap nor leave
it.  What the library does with the layouts on the GPU: the side families' suites and tests/test_gpu_layout_resize.py."""
import pytest

from test_phase_cpu import _host_check


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_carver_offsets_totals_and_bounds_on_the_host(tmp_path, sanitize):
    """4000 seeded piece lists (1 .. 32 pieces; counts 0, 1, 3, 4, 5, 63, 64, 65, 1023; 4-, 8- and 64-byte elements;
    natural or 16-byte alignment), a 33rd piece refused, a zero-count piece that moves nothing, and the three padding rules
    the carver replaced - (n + 4) & ~3 ints, (c + 1) & ~1 doubles, (n + 8) & ~3 ints - at n = 1 .. 5, 63 .. 65, 1023; a
    carver that ignores the alignment argument must get cases wrong (the program fails otherwise)."""
    _host_check(tmp_path, "carve_check", sanitize, "sphx_carve: 0 violations in ")
