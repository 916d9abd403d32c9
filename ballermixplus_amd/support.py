"""Support intervals around each refined maximum: the definition behind --support, and its writer.

--refine replaces a window's grid labels with an off-grid maximum (ballermixplus_amd/refine.py).  --support says how well the
data determine it: for each free coordinate, the range over which the profile of T stays within D of the maximum.  The device
(support_kernel, bmx_ctx_support) implements exactly the rules below; the CPU tests run them on a host restatement of T.

Objective, coordinates, hull.  T, u = ln A, x, v = ln alpha_beta, the free coordinates and the hull are refine.py's.

Centre.  The window's refined point c* as bmx_ctx_refine left it (the grid argmax where the refinement did not improve): natural
values nat* = the refined (A, x, alpha_beta); coordinates c*_k = the grid start's own coordinate where nat*_k is the start's
grid value, else to_coord(k, nat*_k).  Natural values of any point c of the window's searches are
refine.natural_of(c, c*, nat*).  T* is T at c*, evaluated by the search's own arithmetic (not the scan's product-form CLR).
The threshold is L = T* - D.

Profile.  P_k(t) of a free coordinate k at the value t is the maximum over the other free coordinates found by refine.compass
with coordinate k held at t: the same candidate order, strict '>', halving and hull clamping, warm-started from the nuisance
coordinates of the last inside point, with the window's grid-start steps h0 (refine.Setup.start of the scan argmax) as initial
steps, tolerance NUIS_TOL and refine.MAX_ROUNDS rounds.  With no other free coordinate P_k(t) is T at the point.  The search
finds a local maximum, so P is a lower bound on the true profile and the interval may be narrower than the true one.

One end per free k and side s = -1 (lo), +1 (hi):
  walk:    in = c*, d = h0_k.  Repeat (at most MAX_WALK profiles): t = clamp(in_k + s d).  If t == in_k the end is censored at
           the hull.  Else if P_k(t) >= L, in = that profile's point and d <- 2d; otherwise that point is the outside point.
  bisect:  while |out_k - in_k| >= END_TOL[k]: m = in_k + 0.5 (out_k - in_k); P_k(m) warm-started from in; if >= L, in = its
           point, else out = its point.
  report:  the end in_k in natural units; the witness in (three natural values) and its T; the outside point and its T; and
           whether the end is censored (on the hull, or MAX_WALK profiles without leaving the interval).
T_best is the largest T evaluated by any of the window's searches, T* included.  If it exceeds T*, the refined point was not the
maximum; the interval is still relative to T*.

Scope.  Fixed coordinates (--fixX, --fixAlpha, a one-value --listA) have no interval (NA).  Windows that were not refined, or
whose refined CLR is below --supportMin, get an all-NA row.

These are support intervals of a composite likelihood: T treats linked sites as independent, so read as confidence intervals
they are too narrow under linkage disequilibrium.  D (default: the chi-square(1) 95 % point, T being 2 delta ln L) is a support
threshold, not a calibrated coverage level.
"""
import math

import numpy as np

from . import refine

END_TOL = (1e-3, 1e-4, 1e-3)      # u = ln A, x, v = ln alpha_beta
NUIS_TOL = (1e-3, 1e-4, 1e-3)
MAX_WALK = 64
DROP = 3.841458820694124          # chi-square(1) 95 % point
COLUMNS = ('A', 'x', 's')         # coordinate k -> column stem (s: s_hat, alpha_beta)


def value_refusal(drop, min_clr):
    """The message that refuses these values of --supportDrop / --supportMin (None: the flag was not given), or None."""
    if drop is not None and not (math.isfinite(drop) and drop > 0):
        return '--supportDrop takes a finite number > 0.'
    if min_clr is not None and min_clr != min_clr:
        return '--supportMin takes a number.'
    return None


def centre(setup, grid_point, refined_point):
    """(c*, nat*, h0) of a window from its scan argmax (A, x, abeta) and its refined natural values."""
    c0, nat0, h0 = setup.start(*grid_point)
    nat = tuple(float(v) for v in refined_point)
    c = tuple(c0[k] if nat[k] == nat0[k] else refine.to_coord(k, nat[k]) for k in range(3))
    return c, nat, h0


def profile(f, k, t, start, free, lo, hi, h0, tol=NUIS_TOL, max_rounds=refine.MAX_ROUNDS):
    """P_k(t): (point, T, rounds) of the compass search over the free coordinates other than k, from `start` with c_k = t."""
    c = tuple(start[:k]) + (float(t),) + tuple(start[k + 1:])
    nuis = tuple(bool(free[j]) and j != k for j in range(3))
    p, T, rounds, _ = refine.compass(f, c, nuis, lo, hi, h0, tol, max_rounds)
    return p, T, rounds


def one_end(f, k, s, c_star, T_star, L, free, lo, hi, h0):
    """One end of the interval of coordinate k on side s (-1, +1), in coordinates:
    {'end', 'witness', 'witness_T', 'outside', 'outside_T', 'censored', 'rounds', 'evals'} (outside None when censored)."""
    inp, Tin = tuple(c_star), T_star
    out, Tout = None, None
    d = h0[k]
    censored = False
    rounds = evals = 0
    while True:
        if evals == MAX_WALK:
            censored = True
            break
        t = min(max(inp[k] + s * d, lo[k]), hi[k])
        if t == inp[k]:
            censored = True
            break
        p, T, r = profile(f, k, t, inp, free, lo, hi, h0)
        rounds += r
        evals += 1
        if T >= L:
            inp, Tin = p, T
            d *= 2.0
        else:
            out, Tout = p, T
            break
    if not censored:
        while abs(out[k] - inp[k]) >= END_TOL[k]:
            m = inp[k] + 0.5 * (out[k] - inp[k])
            p, T, r = profile(f, k, m, inp, free, lo, hi, h0)
            rounds += r
            evals += 1
            if T >= L:
                inp, Tin = p, T
            else:
                out, Tout = p, T
    return dict(end=inp[k], witness=inp, witness_T=Tin, outside=out, outside_T=Tout, censored=censored, rounds=rounds,
                evals=evals)


def support_window(f, c_star, free, lo, hi, h0, drop=DROP):
    """Every end of one window on the objective f(coordinates) -> T around c*: (T*, T_best, ends) with ends[k][side]
    (side 0: lo, 1: hi) one_end()'s dict in coordinates, or None for a fixed coordinate."""
    best = [-math.inf]

    def g(c):
        T = refine._finite(f(c))
        best[0] = max(best[0], T)
        return T
    T_star = g(tuple(c_star))
    L = T_star - drop
    ends = [[one_end(g, k, s, c_star, T_star, L, free, lo, hi, h0) if free[k] else None for s in (-1, 1)] for k in range(3)]
    return T_star, best[0], ends


def support_natural(T_natural, setup, grid_point, refined_point, drop=DROP):
    """support_window() on T_natural(A, x, abeta) for a window with scan argmax grid_point and refinement refined_point; the
    ends' 'end', 'witness' and 'outside' in natural units."""
    c, nat, h0 = centre(setup, grid_point, refined_point)
    T_star, T_best, ends = support_window(refine.coord_objective(T_natural, c, nat), c, setup.free, setup.lo, setup.hi, h0,
                                          drop)
    for k in range(3):
        for e in ends[k]:
            if e is None:
                continue
            e['witness'] = refine.natural_of(e['witness'], c, nat)
            e['end'] = e['witness'][k]
            if e['outside'] is not None:
                e['outside'] = refine.natural_of(e['outside'], c, nat)
    return T_star, T_best, ends


# ---------------------------------------------------------------------------------------------------------- output

HEADER = 'physPos\tgenPos\tCLR\tx_lo\tx_hi\ts_lo\ts_hi\tA_lo\tA_hi\tCLR_best\tcensored\n'
ORDER = (1, 2, 0)                 # column order of the coordinates: x, s (alpha_beta), A


def output_name(outfile):
    return outfile + '.support.txt'


def format_row(head, clr, lo, hi, censored, T_best):
    """One line of <out>.support.txt: head = (physPos, genPos); lo, hi, censored[k][side] per coordinate k (NaN lo/hi: NA)."""
    vals, cens = [], []
    for k in ORDER:
        for side, v in enumerate((lo[k], hi[k])):
            if v != v:
                vals.append('NA')
                continue
            vals.append(repr(float(v)))
            if censored[k][side]:
                cens.append('%s_%s' % (COLUMNS[k], ('lo', 'hi')[side]))
    return '\t'.join(list(head) + [repr(float(clr))] + vals + [repr(float(T_best)), ','.join(cens) or '.']) + '\n'


def na_row(head):
    return '\t'.join(list(head) + ['NA'] * 9) + '\n'


def write_support(path, main_path, ts, refined_clr, sup):
    """<out>.support.txt: one line per line of the main output, in its order.  The main output's NA rows, and test sites
    whose support was not computed (sup['rounds'] all -1), are all-NA rows.  sup: fetch_support()'s dict."""
    with open(main_path) as f:
        lines = f.readlines()
    out = [HEADER] + [na_row(l.rstrip('\n').split('\t')[:2]) for l in lines[1:]]
    order = ts.order if ts.na_rows else None
    done = np.any(np.asarray(sup['rounds']) >= 0, axis=(1, 2)) if sup is not None else np.zeros(0, dtype=bool)
    for j in np.nonzero(done)[0].tolist():
        pos = 1 + (order[j] if order is not None else j)
        head = lines[pos].rstrip('\n').split('\t')[:2]
        out[pos] = format_row(head, refined_clr[j], sup['lo'][j], sup['hi'][j], sup['censored'][j], sup['T_best'][j])
    with open(path, 'w') as f:
        f.writelines(out)


def support_and_write(ctx, outfile, ts, drop, min_clr):
    """After refine_and_write() of one file on ctx's selected slot: its support intervals into <outfile>.support.txt."""
    if len(ts) == 0:
        write_support(output_name(outfile), outfile, ts, [], None)
        return
    ctx.support(drop, min_clr)
    write_support(output_name(outfile), outfile, ts, ctx.fetch_refined()['clr'], ctx.fetch_support())
