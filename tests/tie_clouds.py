"""Clouds that drive the hinted search's near-tie path on purpose, and a CPU model that predicts how often (test helper,
no test of its own: tests/test_tie_clouds_cpu.py checks the predictions' preconditions, tests/test_gpu_search_ties.py
runs the clouds).

The grouped search (sphx_knn_group.hip) orders 64 fp32 keys per query and certifies every gap between consecutive ranks
against an error window.  A near tie of exactly two consecutive ranks with certain neighbours on both sides becomes an
ENTRY of the tie list, which the tie blocks of the list-mode launch re-order from exact fp64 distances; every other near
tie (a chain of three, a pair across ranks 15|16, 31|32, 47|48: two lanes) makes the query AMBIGUOUS and hands it to the
general kernel.  The tie list has room for npad / 16 + 1024 entries.

The kernel's rule, restated (ranks 0-based, rank 0 the query itself; d2 the exact squared distances in ascending order,
R the query's search radius = hint x rscale):
  keys        floor(d2_fp32 x 2^21 / (1.0002 R^2)): bins of BIN = 2^-21 x 1.0002 R^2
  g[r]        r = 0 .. K: rank r + 1 is listed (inside the radius) and key[r + 1] - key[r] <= win; never for r = 63
              (there is no 65th key)
  entry at r  r < K, g[r], not g[r - 1], not g[r + 1], r % 16 != 15
  ambiguous   some g[r] with r < K is not an entry
  also handed on: fewer than K or more than 64 candidates listed; the K-th too close to the radius

The window depends on a run-time tolerance, tol_rel = 2^-24 (6.93 E / Rc + 7.5) with E the group's tile extent, which the
model does not know.  What it does know (sphx_knn_group.hip, "phase A" and "certify"):
  * a query with tol_rel > TOL_CAP = 0.5e-4 is handed on, so for every query that gets as far as the window
        7.5 x 2^-24 <= tol_rel <= TOL_CAP
  * win = floor(2 tol_rel 2^21) + 3, so 4 <= win <= WIN_MAX = floor(2 TOL_CAP 2^21) + 3 = 212 bins
  * each fp32 d2 lies within tol_rel Rc^2 = tol_rel 2^21 x 1.0002 bins of the truth: at most E_MAX = 104.9 bins; a key is
    a floor of (d2 x a scale rounded to fp32), which moves a difference of two keys by less than 1 + 2 x 2^21 x 2^-23 =
    1.25 bins more (FLOOR_SLACK = 1.5 taken)
so a gap between two listed ranks is classified only where every admissible tolerance gives the same answer:
  * true gap < IN_BINS = 1 bin:  key difference < 1 + 2 e + 1.5 with e = tol_rel 2^21 x 1.0002, an integer, hence
    <= floor(2 tol_rel 2^21) + 3 = win for that very tol_rel: INSIDE every window
  * true gap > OUT_BINS = WIN_MAX + 2 E_MAX + 2 FLOOR_SLACK = 424.8 bins:  key difference > gap - 2 E_MAX - 1.5 > WIN_MAX:
    OUTSIDE every window
  * anything between: unclassified; a query with an unclassified gap among r = 0 .. K is UNDECIDED.
Whether rank r + 1 is listed is fuzzy as well: a candidate truly inside R is always listed, one beyond LIST_OUT R^2 never
(packed-fp32 form: fp32 d2 <= 1.0002 R^2, i.e. d2 <= (1.0002 + TOL_CAP) R^2; matrix-core form: d2 - R^2 (1 + 2e-3) <
kappa E^2 <= 1.75e-3 R^2, i.e. d2 < 1.00375 R^2; LIST_OUT = 1.004 covers both).  Between the two a candidate may be
listed with its key clamped to the last bin, so a gap that ends there is classified (as outside) only if it is wide AND
begins below NEAR_EDGE R^2 = (1 - 1e-3) R^2, 2097 bins under the radius: further than OUT_BINS under the lowest key a
listed candidate beyond R can get ((1 / 1.0002 - TOL_CAP) 2^21 - 1 bins, 525 under the top).
"""
import numpy as np

BINS = 2097152.0                 # 2^21 bins up to ACC R^2
ACC = 1.0002                     # the acceptance pad of the keys' scale
TOL_CAP = 0.5e-4
WIN_MAX = float(np.floor(2.0 * TOL_CAP * BINS)) + 3.0
E_MAX = TOL_CAP * BINS * ACC
FLOOR_SLACK = 1.5
IN_BINS = 1.0
OUT_BINS = WIN_MAX + 2.0 * E_MAX + 2.0 * FLOOR_SLACK
LIST_OUT = 1.004
NEAR_EDGE = 1.0 - 1e-3
MAX_LISTED = 64

BOX = 2e17                       # the base points: (rand - 0.5) x BOX
TWIN = 1e-9                      # a twin's displacement, in mean spacings of the base points


def tie_capacity(n):
    """Room in the tie list of a search over n particles (sphx_knn.hip: npad / 16 + 1024, npad = n rounded up to 64)."""
    return (n + 63) // 64 * 64 // 16 + 1024


def rscale_for(K):
    """Hint scale per K: about min(1.3 K, 62) candidates inside R = rscale x h (count ~ rscale^3 K), and never below
    1.004 - for K = 63 and 64 the radius is barely above h, the list all but full."""
    return max(1.004, (min(1.3 * K, 62.0) / K) ** (1.0 / 3.0))


# ---- generators (all seeded) ----------------------------------------------------------------------------------------
def _base(m, rs):
    return (rs.rand(m, 3) - 0.5) * BOX


def _copies(pts, rs, spacing, scale=TWIN):
    """One displaced copy of every point of pts: scale x spacing in a random direction (scale = 0: coincident)."""
    u = rs.normal(size=pts.shape)
    u /= np.linalg.norm(u, axis=1)[:, None]
    return pts + u * (scale * spacing)


def _spacing(m):
    return BOX / m ** (1.0 / 3.0)


def all_twin(m, seed=11):
    """Every point twinned (2 m particles): pairs at ranks (0,1), (2,3), ...  Even K ends between two pairs, odd K puts
    the last pair across the K boundary."""
    rs = np.random.RandomState(seed)
    b = _base(m, rs)
    return np.ascontiguousarray(np.concatenate([b, _copies(b, rs, _spacing(m))]))


def half_twin(m, seed=12):
    """Each point twinned with probability 0.5: every alignment of the pairs occurs, ranks 15|16, 31|32, 47|48 included."""
    rs = np.random.RandomState(seed)
    b = _base(m, rs)
    pick = rs.rand(m) < 0.5
    return np.ascontiguousarray(np.concatenate([b, _copies(b[pick], rs, _spacing(m))]))


def sparse_twin(n, seed=13, p=0.001, scale=TWIN):
    """Twinned with probability 0.001: isolated pairs at arbitrary ranks, far under the tie list's capacity."""
    rs = np.random.RandomState(seed)
    b = _base(n, rs)
    pick = rs.rand(n) < p
    return np.ascontiguousarray(np.concatenate([b, _copies(b[pick], rs, _spacing(n), scale)]))


def coincident(n, seed=14):
    """sparse_twin with displacement exactly 0: exact fp64 ties, broken by index."""
    return sparse_twin(n, seed=seed, scale=0.0)


def triplets(n, seed=15, p=0.01):
    """A fraction p of the points in threes: chains of three near ties, which must fail over."""
    rs = np.random.RandomState(seed)
    b = _base(n, rs)
    pick = rs.rand(n) < p
    s = _spacing(n)
    return np.ascontiguousarray(np.concatenate([b, _copies(b[pick], rs, s), _copies(b[pick], rs, s)]))


def clustered_twin(n, K, seed=16, fill=2.2):
    """Every point inside one small ball (around the origin) twinned, the rest not.  The ball holds as many base points as
    give the model's lower bound about fill x the tie list's capacity in entries: a query deep inside it carries an entry
    at every other rank, (K + 1) // 2 of them; one whose K nearest reach out of the ball fewer, one outside whose K
    nearest reach in a few - the two rims roughly cancel.  The model can decide a smaller share of the queries the larger
    K is (one unclassified gap among K + 1 leaves a query out of the lower bound: about K / 50 of them more for every one
    kept, by the clouds here), so the ball grows by that factor.  tests/test_tie_clouds_cpu.py checks the outcome with the
    model: a lower bound of 1.5 .. 3 x the capacity, and at least 90 % of the decided queries without an entry."""
    rs = np.random.RandomState(seed)
    b = _base(n, rs)
    per_query = (K + 1) // 2
    nball = int(np.ceil(fill * (1.0 + K / 50.0) * tie_capacity(n) / (2.0 * per_query)))
    assert nball <= n // 25, "the ball would hold more than 4 % of the cloud"
    inside = np.argsort(np.sum(b * b, axis=1))[:nball]
    return np.ascontiguousarray(np.concatenate([b, _copies(b[inside], rs, _spacing(n))]))


# ---- the model ------------------------------------------------------------------------------------------------------
def predict(points, K, R):
    """What the grouped search must do with every query of `points` searched for K neighbours inside radii R (array or
    scalar).  -> dict:
      lower        entries of the CLEAN queries: decided, unambiguous, K .. 64 candidates listed whatever the tolerance -
                   queries the kernel certifies unless their whole group gives up (tile or row caps, radius spread,
                   tolerance), each reserving exactly these entries
      upper        every gap r < K that could be inside some window, wherever it sits and whatever becomes of its query
      per_rank     (K,) the lower bound's entries by rank
      max_per_query  most entries of one clean query
      clean, undecided, ambiguous, certain_fallback   (N,) bool; certain_fallback: handed on whatever the tolerance
                   (decided and ambiguous, or surely fewer than K / more than 64 listed)
      straddle_only  (N,) bool: decided queries that are ambiguous ONLY because of pairs across a lane boundary (r % 16 = 15)
      entries      (N,) entries per query as far as decided (0 for undecided queries)
    """
    from scipy.spatial import cKDTree
    pts = np.ascontiguousarray(points, dtype=np.float64)
    n = len(pts)
    R = np.broadcast_to(np.asarray(R, dtype=np.float64), (n,))
    m = min(max(K + 2, MAX_LISTED + 1), n)
    d, _ = cKDTree(pts).query(pts, m, 0.0, 2)
    d2 = d * d                                              # (relative error 2^-52: nothing against a bin of 2^-21)
    if m < max(K + 2, MAX_LISTED + 1):
        d2 = np.concatenate([d2, np.full((n, max(K + 2, MAX_LISTED + 1) - m), np.inf)], axis=1)
    R2 = (R * R)[:, None]
    binw = ACC * R2 / BINS
    lo, hi = d2[:, :K + 1], d2[:, 1:K + 2]                  # ranks r and r + 1, r = 0 .. K
    with np.errstate(invalid="ignore"):
        gap = (hi - lo) / binw
    listed_sure = hi <= R2
    unlisted_sure = hi > LIST_OUT * R2
    g_true = listed_sure & (gap < IN_BINS)
    g_false = unlisted_sure | ((gap > OUT_BINS) & (listed_sure | (lo <= NEAR_EDGE * R2)))
    if K + 1 > 63:
        g_true[:, 63:] = False                              # r = 63: the kernel has no 65th key
        g_false[:, 63:] = True
    g_maybe = ~g_false                                      # true or unclassified
    undecided = (~g_true & ~g_false).any(axis=1)
    # entries and ambiguity (meaningful for decided queries, where g_true = ~g_false)
    g = g_true
    r = np.arange(K)
    prev = np.concatenate([np.zeros((n, 1), bool), g[:, :K - 1]], axis=1)
    nxt = g[:, 1:K + 1]
    entry = g[:, :K] & ~prev & ~nxt & (r % 16 != 15)[None, :]
    amb_at = g[:, :K] & ~entry
    ambiguous = amb_at.any(axis=1)
    # ... ambiguous only through lane-straddling pairs: with the rule r % 16 != 15 dropped nothing is left over
    entry_nolane = g[:, :K] & ~prev & ~nxt
    straddle_only = ~undecided & ambiguous & ~(g[:, :K] & ~entry_nolane).any(axis=1)
    # candidates listed: surely >= K (the K-th truly inside R, which also keeps it clear of the radius: key[K - 1] <=
    # (1 / 1.0002 + TOL_CAP) 2^21 < the kernel's `safe` = (1 - 2 TOL_CAP / 1.0002) 2^21 - 2), surely <= 64
    enough = d2[:, K - 1] <= R2[:, 0]
    not_over = d2[:, MAX_LISTED] > LIST_OUT * R2[:, 0]
    surely_short = d2[:, K - 1] > LIST_OUT * R2[:, 0]
    surely_over = d2[:, MAX_LISTED] <= R2[:, 0]
    clean = ~undecided & ~ambiguous & enough & not_over
    certain_fallback = (~undecided & ambiguous) | surely_short | surely_over
    per_query = entry.sum(axis=1)
    return dict(lower=int(per_query[clean].sum()), upper=int(g_maybe[:, :K].sum()),
                per_rank=entry[clean].sum(axis=0), max_per_query=int(per_query[clean].max()) if clean.any() else 0,
                clean=clean, undecided=undecided, ambiguous=ambiguous & ~undecided, certain_fallback=certain_fallback,
                straddle_only=straddle_only, entries=np.where(undecided, 0, per_query))


def exact_h(points, K):
    """The exact K-th-neighbour distance (the query itself is the first), as the suite's other search tests take it."""
    from oracle import sph_oracle as orc
    return orc.neighbors(points, np.inf, K, eps=0.0)[4]


# ---- the clouds and K the tests use, each made and predicted once per process -----------------------------------------
SIZES = dict(all_twin=6000, half_twin=8000, sparse_twin=30000, coincident=30000, triplets=20000, clustered_twin=20000)
K_ALL = (7, 16, 17, 33, 40, 63, 64)          # all_twin, half_twin: exactness at every alignment of pairs and lanes
K_SOME = (7, 16, 33, 40, 64)                 # sparse_twin, coincident, triplets: exactness
K_UNDER = (7, 14, 40)                        # the under-capacity counter test: neither K - 1 nor K - 2 is a lane's last
                                             # rank, so both h-rewriting ranks can hold entries
K_UNDER_PROVEN = (7, 14, 16)                 # ... where the model's UPPER bound is below the capacity as well (it grows as
                                             # K^2 - every unclassified gap of the untwinned bulk counts - and passes the
                                             # capacity near K = 18: at 33 and 40 only the GPU can say that the list held)
K_FUSED = (16, 33, 40)                       # the fused step
K_CLUSTER = (16, 33, 40)                     # clustered_twin: device API (16, 40) and fused step.  Not 7: the radii of a
                                             # group's 64 queries then scatter beyond the 1.5 x the grouped kernel sizes one
                                             # tile for, and four queries in ten of ANY cloud are handed on for that alone -
                                             # the cloud's point is an overflow with most rows certified
_cache = {}


def cloud(name, K=None, seed=None):
    """The test cloud `name` (clustered_twin is sized per K); seed: another draw of the same kind and size."""
    key = ("cloud", name, K if name == "clustered_twin" else None, seed)
    if key not in _cache:
        kw = {} if seed is None else dict(seed=seed)
        gen = globals()[name]
        _cache[key] = gen(SIZES[name], K, **kw) if name == "clustered_twin" else gen(SIZES[name], **kw)
    return _cache[key]


def hints(name, K, seed=None):
    """The exact radii of cloud(name, K, seed): the hints of the GPU tests and what their results must equal."""
    key = ("h", name, K, seed)
    if key not in _cache:
        _cache[key] = exact_h(cloud(name, K, seed), K)
    return _cache[key]


def prediction(name, K):
    """predict() for cloud(name, K) searched with R = rscale_for(K) x the exact radii."""
    key = ("pred", name, K)
    if key not in _cache:
        _cache[key] = predict(cloud(name, K), K, rscale_for(K) * hints(name, K))
    return _cache[key]
