"""NumPy restatement of the closing block of the reference's time loop, code_running.py:493-540: the global length scale
d and the adapted sizes, line by line, with what include/sphx.h (sphx_length_scale, sphx_adapt_sizes) defines where the
driver leaves it open:

  * the percentile as TWO ORDER STATISTICS and a lerp (two_stat_percentile): what np.percentile's method `linear` does
    (numpy/lib/_function_base_impl.py: _quantile, _get_indexes, _lerp); test_scale_cpu.py holds it to np.percentile's bits;
  * no slow row: ValueError; a NaN dist_sq among the slow rows: NaN, the rows counted;
  * an entry of the list outside [0, n) is ignored and counted; a row nobody lists counts 0;
  * densities_0 None or of another length: new_smoothing = 1. and no bonus (drv:534-535).

Nothing here is tuned to the library's output: every line follows the driver's statement or the header's rule."""
import numpy as np

V_MAX = 80000.                   # drv:518
Q = 90.                          # drv:518
FILL = 0.9                       # drv:521
COUNTS = ("bonus", "capped", "nan_to_num", "missing")


def two_stat_percentile(vals, qf):
    """-> (lo, hi, a, b, result): np.percentile(vals, 100 qf), method linear, from the order statistics of rank lo and hi."""
    vals = np.asarray(vals, dtype=np.float64)
    M = vals.shape[0]
    if M < 1:
        raise ValueError("no value")
    vi = (M - 1) * qf
    if vi >= M - 1:
        lo = hi = M - 1
    else:
        lo = int(np.floor(vi))
        hi = lo + 1
    g = np.float64(vi - lo)
    s = np.sort(vals)                                   # (NaN last)
    a, b = s[lo], s[hi]
    with np.errstate(all="ignore"):
        diff = b - a
        r = a + diff * g
        if g >= 0.5:
            r = b - diff * (1 - g)
    if np.isnan(s[-1]):
        r = np.float64(np.nan)
    return lo, hi, a, b, r


def length_scale(points, velocities, N_INT_PER_PARTICLE, q=Q, v_max=V_MAX, fill=FILL):
    """drv:493, 515-521 -> dict: n_slow, n_nan, lo, a, b, max_dist, d."""
    points = np.asarray(points, dtype=np.float64)
    velocities = np.asarray(velocities, dtype=np.float64)
    with np.errstate(all="ignore"):
        vel_condition = np.sum(velocities ** 2, axis=1)                                          # drv:493
        dist_sq = np.sum(points ** 2, axis=1)                                                    # drv:515
        slow = vel_condition < v_max ** 2
        M = int(np.count_nonzero(slow))
        if M == 0:
            raise ValueError("no row is slower than v_max")
        lo, hi, a, b, max_dist = two_stat_percentile(dist_sq[slow], np.true_divide(q, 100))      # drv:518
        V_new = max_dist ** (3. / 2.)                                                            # drv:520
        d = (V_new / M / fill * N_INT_PER_PARTICLE) ** (1. / 3.)                                 # drv:521
    return dict(n_slow=M, n_nan=int(np.count_nonzero(np.isnan(dist_sq[slow]))), lo=lo, a=float(a), b=float(b),
                max_dist=float(max_dist), d=float(d))


def reverse_counts(neighbor, n):
    """-> (exp_neighbor_count, num_nontrivial, missing): drv:527-530 and nsc:545 over the entries inside [0, n)."""
    nb = np.asarray(neighbor, dtype=np.int64)
    ok = (nb >= 0) & (nb < n)
    return (np.bincount(nb[ok], minlength=n).astype(np.int64), np.count_nonzero(ok, axis=1).astype(np.int64),
            int(np.count_nonzero(~ok)))


def adapt_sizes(neighbor, densities, densities_0, sizes, particle_type, d, raise_factor):
    """drv:527-538 -> dict: sizes, exp_neighbor_count, num_nontrivial, new_smoothing, counts."""
    densities = np.asarray(densities, dtype=np.float64)
    particle_type = np.asarray(particle_type, dtype=np.float64)
    sizes = np.array(sizes, dtype=np.float64)
    n = sizes.shape[0]
    exp_neighbor_count, num_nontrivial, missing = reverse_counts(neighbor, n)
    bonus = fixed = 0
    with np.errstate(all="ignore"):
        if densities_0 is not None and len(densities_0) == len(densities):                       # drv:532
            densities_0 = np.asarray(densities_0, dtype=np.float64)
            x = -(densities - densities_0) / (3 * densities)
            y = np.nan_to_num(x)
            few = exp_neighbor_count + num_nontrivial - 1 < 2
            new_smoothing = (np.exp(y) * 2) / 2. + few * 0.1                                     # drv:533
            bonus = int(np.count_nonzero(few))
            fixed = int(np.count_nonzero(~(y == x)))
        else:
            new_smoothing = 1.                                                                   # drv:535
        sizes[particle_type == 0] = (new_smoothing * sizes)[particle_type == 0]                  # drv:536
        cap = (particle_type == 0) & (sizes > d)
        sizes[cap] = d                                                                           # drv:537
        sizes[particle_type == 2] = d / raise_factor ** (1. / 3.)                                # drv:538
    return dict(sizes=sizes, exp_neighbor_count=exp_neighbor_count, num_nontrivial=num_nontrivial,
                new_smoothing=np.broadcast_to(np.float64(new_smoothing), (n,)).copy(),
                counts=dict(bonus=bonus, capped=int(np.count_nonzero(cap)), nan_to_num=fixed, missing=missing))


def same_bits(x, y):
    """x and y are the same doubles, every NaN counting as one value."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and bool(np.all((x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))))
