"""CPU checks of what tests/test_gpu_search_ties.py rests on: the tie clouds' predicted entry counts (tests/tie_clouds.py:
a restatement of the grouped search's near-tie rule over exact distances) put each cloud in the regime its GPU test
claims, and the rule that fills the tie list's slots (kg_tie_slots, sphx_knn_group.h) keeps its invariant under random
interleavings of the reservations - replayed by a stand-alone host program, with and without sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tie_clouds as tc
from conftest import ROOT


def _pred(name, K):
    pts = tc.cloud(name, K)
    return pts, tc.prediction(name, K)


# ---- the model's thresholds come out of the kernel's constants ----
def test_window_thresholds_are_the_derived_ones():
    assert tc.WIN_MAX == 212.0                                   # floor(2 x 0.5e-4 x 2^21) + 3
    assert 104.8 < tc.E_MAX < 104.9
    assert 424.0 < tc.OUT_BINS < 430.0
    assert tc.IN_BINS == 1.0
    assert tc.tie_capacity(20000) == 20032 // 16 + 1024
    assert tc.tie_capacity(64) == 4 + 1024 and tc.tie_capacity(65) == 8 + 1024
    for K in (7, 16, 17, 33, 40):
        assert abs(tc.rscale_for(K) ** 3 - 1.3) < 1e-12
    assert tc.rscale_for(63) == 1.004 and tc.rscale_for(64) == 1.004


def test_model_on_hand_made_rows():
    """Five queries' worth of gaps laid out by hand along a line (distances from the first point), K = 4: an isolated
    pair, a chain of three, an unclassified gap, a pair across the K boundary with b the unlisted (K+1)-th, and no tie."""
    K = 4
    R = 1.0
    binw = tc.ACC * R * R / tc.BINS

    def row(d2):
        # points on the x axis at sqrt(d2); only the FIRST point's row is looked at, the others sit where they must
        return np.stack([np.sqrt(np.asarray(d2, dtype=np.float64)), np.zeros(len(d2)), np.zeros(len(d2))], axis=1)

    far = [4.0 + 0.1 * q for q in range(70)]                     # (ranks 6 .. : beyond the radius)
    cases = {
        "pair": [0.0, 0.1, 0.1 + 0.5 * binw, 0.3, 0.5, 0.7],
        "chain": [0.0, 0.1, 0.1 + 0.4 * binw, 0.1 + 0.8 * binw, 0.5, 0.7],
        "unclassified": [0.0, 0.1, 0.1 + 100 * binw, 0.3, 0.5, 0.7],
        "across_K": [0.0, 0.1, 0.2, 0.3, 0.3 + 0.5 * binw, 0.7],
        "none": [0.0, 0.1, 0.2, 0.3, 0.5, 0.7],
    }
    got = {}
    for name, d2 in cases.items():
        m = tc.predict(row(d2 + far), K, R)
        got[name] = {k_: (v[0] if isinstance(v, np.ndarray) and v.dtype == bool else v) for k_, v in m.items()}
        got[name]["e0"] = int(m["entries"][0])
    assert got["pair"]["clean"] and got["pair"]["e0"] == 1
    assert got["chain"]["ambiguous"] and got["chain"]["certain_fallback"] and not got["chain"]["clean"]
    assert got["unclassified"]["undecided"] and not got["unclassified"]["clean"] and got["unclassified"]["e0"] == 0
    assert got["across_K"]["clean"] and got["across_K"]["e0"] == 1            # r = K - 1 = 3
    assert got["none"]["clean"] and got["none"]["e0"] == 0
    # a pair across a lane boundary: ranks 15 | 16 with K = 20
    d2 = [0.01 * q for q in range(15)] + [0.2, 0.2 + 0.5 * binw] + [0.3 + 0.01 * q for q in range(6)]
    m = tc.predict(row(d2 + far), 20, R)
    assert m["straddle_only"][0] and m["certain_fallback"][0] and not m["clean"][0]


# ---- the regimes ----
@pytest.mark.parametrize("name", ["sparse_twin", "coincident"])
@pytest.mark.parametrize("K", sorted(set(tc.K_UNDER + tc.K_FUSED)))
def test_sparse_clouds_reach_the_h_rewriting_ranks(name, K):
    """The lower bound holds at least 10 entries at each of the two h-rewriting ranks, K - 1 (b the unlisted (K+1)-th) and
    K - 2, for every K whose GPU test asserts counters.  A lane's last rank (r % 16 = 15) can hold no entry by the kernel's
    rule (the pair would span two lanes): the fused step's K = 16 and K = 33 have only one of the two ranks, K_UNDER both."""
    pts, m = _pred(name, K)
    print(name, K, "N", len(pts), "capacity", tc.tie_capacity(len(pts)), "lower", m["lower"], "upper", m["upper"],
          "rank K-1", m["per_rank"][K - 1], "rank K-2", m["per_rank"][K - 2], "clean %.3f" % m["clean"].mean())
    for r in (K - 1, K - 2):
        if r % 16 == 15:
            assert K not in tc.K_UNDER and m["per_rank"][r] == 0
        else:
            assert m["per_rank"][r] >= 10, (r, m["per_rank"][r])
    assert m["max_per_query"] >= 1


@pytest.mark.parametrize("name", ["sparse_twin", "coincident"])
@pytest.mark.parametrize("K", tc.K_UNDER_PROVEN)
def test_sparse_clouds_stay_under_the_capacity_whatever_the_tolerance(name, K):
    """Every gap that could lie inside some window, counted wherever it sits, is fewer than the tie list holds."""
    pts, m = _pred(name, K)
    assert m["lower"] <= m["upper"] < tc.tie_capacity(len(pts)), (m["lower"], m["upper"], tc.tie_capacity(len(pts)))


@pytest.mark.parametrize("K", tc.K_ALL)
def test_all_twin_overflows(K):
    pts, m = _pred("all_twin", K)
    cap = tc.tie_capacity(len(pts))
    print("all_twin", K, "lower", m["lower"], "capacity", cap, "clean %.3f" % m["clean"].mean())
    assert m["lower"] > 10 * cap
    # even K ends between two pairs (rank K - 2 | K - 1 is one), odd K puts the last pair across the K boundary
    assert m["per_rank"][K - 2 if K % 2 == 0 else K - 1] > 1000
    assert m["per_rank"][K - 1 if K % 2 == 0 else K - 2] == 0


@pytest.mark.parametrize("K", tc.K_CLUSTER)
def test_clustered_twin_overflows_with_most_queries_untouched(K):
    pts, m = _pred("clustered_twin", K)
    cap = tc.tie_capacity(len(pts))
    decided = ~m["undecided"]
    none = float(((m["entries"] == 0) & decided).sum()) / decided.sum()
    print("clustered_twin", K, "lower", m["lower"], "= %.2f x capacity" % (m["lower"] / cap), "decided queries without an entry %.3f" % none,
          "certain fallbacks %.3f" % m["certain_fallback"].mean())
    assert 1.5 * cap <= m["lower"] <= 3.0 * cap
    assert none >= 0.9
    assert m["certain_fallback"].mean() < 0.05


@pytest.mark.parametrize("K", [16, 17, 33, 40, 63, 64])
def test_half_twin_has_lane_straddling_pairs(K):
    """Decided queries that are ambiguous ONLY because a pair sits across ranks 15|16, 31|32 or 47|48 (K = 7 has no lane
    boundary below K)."""
    _, m = _pred("half_twin", K)
    print("half_twin", K, "straddle-only", m["straddle_only"].sum(), "clean", m["clean"].sum(), "lower", m["lower"])
    assert m["straddle_only"].sum() >= 100
    assert m["lower"] > 0 and (m["per_rank"] > 0).sum() >= min(K, 60) // 2      # entries at many ranks


def test_triplets_are_handed_on():
    pts, m = _pred("triplets", 16)
    assert m["certain_fallback"].sum() >= 0.1 * len(pts)         # chains: ambiguous whatever the tolerance
    assert m["lower"] < 50


# ---- the slot rule, replayed on the host ----
def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tie_slot_rule_keeps_every_walked_slot_written(tmp_path, sanitize):
    """tests/host/tie_slots_check.cpp: random interleavings of the four lanes' reservations around the capacity (one entry
    per lane, up to eight, a crossing that lands exactly on the capacity).  kg_tie_slots must leave every slot below
    min(count, cap) written exactly once, real only for certified queries, nothing at or beyond cap; the rule the kernel
    had before must break that (the program fails otherwise)."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "tie_slots_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        # (GCC links the sanitizer runtimes dynamically by default, and they then insist on being the first library the
        #  process loads; linked into the program itself they do not care what else the environment loads)
        ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in ver.lower():
            flags += ["-static-libasan", "-static-libubsan"]
    res = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "tie_slots_check.cpp")],
                         capture_output=True, text=True)
    if res.returncode != 0 and sanitize and ("asan" in res.stderr or "ubsan" in res.stderr or "sanitize" in res.stderr):
        pytest.skip("this compiler has no sanitizer runtimes: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe, "3000"], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    assert "kg_tie_slots: 0 violations" in out
    former = [ln for ln in out.splitlines() if ln.startswith("former rule:")]
    assert former and int(former[0].split()[2]) > 0              # the parent's rule does break the invariant
