#!/usr/bin/env python3
"""Generate tests/golden/cool_<case>.npz: the reference's rad_cooling (nsc:1019-1176) on seeded inputs.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  It loads the reference the way
make_golden.load_reference does (an in-memory Python-2 -> Python-3 transform; no reference text is stored) with the
two repairs of SURVEY Appendix B Q14 applied in memory: the `np.min(` of the lines that start `frac_rec_e = np.min(`
and `frac_rec_H_neut = np.min(` becomes `np.minimum(` - exactly one hit each, asserted.  As committed those lines
raise TypeError (0.9999 is taken as `axis`).

The particles come from the existing fixtures <case>.npz (not duplicated here): positions, masses, particle_type, the
neighbour list nb_idx, loop_d (assigned to the module global d, as the driver does).  Their f_un is neutral (0.86 /
0.14): every output would be zero.  So a seeded ionised composition is drawn for the gas:
    f0, f2 ~ U(0.1, 0.5), f1 = 0.14, f3 ~ U(0, 0.3), f4 ~ U(0, 0.05), f5 = f3 + f4, rows normalised, dust and star rows
    kept; then FORCED rows: two whole neighbourhoods (a gas particle and every member of its row) get f5 = 0 - rows
    whose electron sum is empty - five more gas particles f5 = 0 and five f5 = 1e-11 U(0, 1);
    T = 10^U(1, 4.5);  mu_array from the drawn composition (code_running.py:162);  dt = dt_0.
Stored: the drawn inputs, the three results, per row the six scalars of nsc:1088-1097 and num_e taken from the frame's
locals at nsc:1110 (sys.settrace; f_* through nan_to_num as the scatter reads them, the energies as they are), the
constants, the versions.

Conditions on the fixture asserted here (conditions, not thresholds; change the seed if one fails):
  some particle on each side of mf2 > 0.9999 (nsc:1124), none at 0.9999 exactly; some with f5 < 1e-10 (nsc:1126);
  some contributing row with num_e = 0.

Usage:  python tests/golden/make_golden_cool.py
"""
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402

CASES = [("sphere_dust_n2048_k40", 6101), ("condensed_n1024_k40", 6102)]
REPAIRS = ("frac_rec_e = np.min(", "frac_rec_H_neut = np.min(")
SCATTER_LINE = "rel_array[neighbor[j]] +="
ROW_LOCALS = ("frac_rec_H_neut", "frac_rec_H", "frac_rec_He", "frac_rec_e", "H_effect_energy", "He_effect_energy")


def load_reference_repaired():
    """-> (module, line number of the row loop's last statement)."""
    os.environ.setdefault("MPLBACKEND", "Agg")
    warnings.simplefilter("ignore")
    from lib2to3 import refactor
    src = open(REF).read().expandtabs(8)
    if not src.endswith("\n"):
        src += "\n"
    lines = src.split("\n")
    for head in REPAIRS:
        hits = [i for i, l in enumerate(lines) if l.strip().startswith(head)]
        assert len(hits) == 1, (head, hits)
        assert lines[hits[0]].count("np.min(") == 1
        lines[hits[0]] = lines[hits[0]].replace("np.min(", "np.minimum(")
    hits = [i for i, l in enumerate(lines) if l.strip().startswith(SCATTER_LINE)]
    assert len(hits) == 1, hits
    src3 = str(refactor.RefactoringTool(["lib2to3.fixes.fix_print"]).refactor_string("\n".join(lines), "nsc"))
    assert src3.split("\n")[hits[0]].strip().startswith(SCATTER_LINE)
    mod = types.ModuleType("nsc_ref_cool")
    exec(compile(src3, mod.__name__, "exec"), mod.__dict__)
    return mod, hits[0] + 1


def call_capturing_rows(fn, lineno, n, *args):
    """fn(*args) -> (result, table (n,6), num_e (n,), contributes (n,)): the row loop's locals, taken each time the
    frame reaches `lineno` (the last statement of the loop body)."""
    code = fn.__code__
    table = np.zeros((n, 6)); num_e = np.full(n, -1.0); contrib = np.zeros(n, np.int8)

    def local(frame, event, arg):
        if event == "line" and frame.f_lineno == lineno:
            loc = frame.f_locals
            j = int(loc["j"])
            row = [float(loc[nm]) for nm in ROW_LOCALS]
            table[j, :4] = np.nan_to_num(np.array(row[:4]))
            table[j, 4:] = row[4:]
            num_e[j] = float(loc["num_e"])
            contrib[j] = 1
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None

    sys.settrace(tracer)
    try:
        res = fn(*args)
    finally:
        sys.settrace(None)
    return res, table, num_e, contrib


def draw(g, nsc, seed):
    rs = np.random.RandomState(seed)
    pt = g["particle_type"]
    nb = g["nb_idx"].astype(np.int64)
    n = pt.shape[0]
    gas = pt == 0
    f = np.array(g["f_un"], dtype=np.float64)
    S = f.shape[1]
    fg = np.zeros((n, S))
    fg[:, 0] = rs.uniform(0.1, 0.5, n); fg[:, 2] = rs.uniform(0.1, 0.5, n); fg[:, 1] = 0.14
    fg[:, 3] = rs.uniform(0.0, 0.3, n); fg[:, 4] = rs.uniform(0.0, 0.05, n); fg[:, 5] = fg[:, 3] + fg[:, 4]
    fg /= np.sum(fg, axis=1)[:, None]
    f[gas] = fg[gas]
    gi = np.nonzero(gas)[0]
    pick = rs.choice(gi, 12, replace=False)
    hoods = np.unique(nb[pick[:2]].ravel())
    hoods = hoods[(hoods < n)]
    hoods = hoods[gas[hoods]]
    f[hoods, 5] = 0.0
    f[pick[2:7], 5] = 0.0
    f[pick[7:12], 5] = 1e-11 * rs.uniform(0.0, 1.0, 5)
    T = 10.0 ** rs.uniform(1.0, 4.5, n)
    mu = np.sum(f * nsc.mu_specie, axis=1) / np.sum(f, axis=1)
    return f, T, mu, pick


def make(nsc, lineno, case, seed):
    g = dict(np.load(os.path.join(HERE, case + ".npz"), allow_pickle=False))
    pts, mass, pt, sizes = g["points"], g["mass"], g["particle_type"], g["nb_h"]
    nb = g["nb_idx"].astype(np.int64)
    n = pts.shape[0]
    f_un, T, mu, pick = draw(g, nsc, seed)
    dt = float(nsc.dt_0)
    nsc.d = float(g["loop_d"])
    cross = np.ones(n)
    keep = [a.copy() for a in (pts, pt, mass, f_un, nb, mu, T)]
    sink = io.StringIO()                       # the two mass-budget prints
    with contextlib.redirect_stdout(sink), np.errstate(all="ignore"):
        (final, energy, rec), table, num_e, contrib = call_capturing_rows(
            nsc.rad_cooling, lineno, n, pts, pt, mass, sizes, cross, f_un, nb, mu, T, dt)
    for a, b in zip(keep, (pts, pt, mass, f_un, nb, mu, T)):
        assert np.array_equal(a, b), "the reference modified an input"
    final, energy, rec = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (final, energy, rec))
    assert final.shape == f_un.shape and energy.shape == (n,) and rec.shape == f_un.T.shape
    assert np.all(np.isfinite(final)) and np.all(np.isfinite(energy)) and np.all(np.isfinite(rec))
    # the conditions (mf2 as nsc:1118-1123 forms it from the results: rec_array rows 3, 4 are returned as used there)
    f = np.nan_to_num(f_un)
    with np.errstate(all="ignore"):
        mf2 = np.maximum(np.nan_to_num(f[:, 5] * rec[3] / f[:, 3]), np.nan_to_num(f[:, 5] * rec[4] / f[:, 4]))
    above, below, at = int(np.sum(mf2 > 0.9999)), int(np.sum(mf2 < 0.9999)), int(np.sum(mf2 == 0.9999))
    tiny = int(np.sum(f[:, 5] < 1e-10))
    empty = int(np.sum((contrib == 1) & (num_e == 0.0)))
    out = dict(f_un=f_un, T=T, mu_array=mu, dt=np.float64(dt), d=np.float64(nsc.d), forced=pick.astype(np.int64),
               final_comp=final, energy=energy, rec_array=rec, row_table=table, row_num_e=num_e, row_contributes=contrib,
               const_k=np.float64(nsc.k), const_m_h=np.float64(nsc.m_h), const_m_0=np.float64(nsc.m_0))
    import scipy
    out["versions"] = np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "python " + sys.version.split()[0]])
    path = os.path.join(HERE, "cool_" + case + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d rows contribute, %d with num_e = 0; mf2 above / below / at 0.9999: %d / %d / %d; f5 < 1e-10: %d; "
          "energy != 0 on %d, rec[5] max %.6g, rec[2] max %.3g; %d bytes"
          % (path, int(contrib.sum()), empty, above, below, at, tiny, int(np.count_nonzero(energy)), rec[5].max(),
             rec[2].max(), size))
    assert size <= 1000000, "fixture over the size limit"
    assert above > 0 and below > 0 and at == 0, "no particle on one side of mf2 > 0.9999 (or one at it): change the seed"
    assert tiny > 0 and empty > 0, "no particle with f5 < 1e-10, or no row with an empty electron sum: change the seed"


def main():
    if not os.path.exists(REF):
        print("reference not present: nothing to do")
        return 0
    nsc, lineno = load_reference_repaired()
    for case, seed in CASES:
        make(nsc, lineno, case, seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
