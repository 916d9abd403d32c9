"""Off-grid refinement of each window's maximum likelihood: the definition behind --refine, and its writer.

The scan maximises T over a grid; its x_hat, s_hat (alpha_beta) and A_hat are grid labels.  --refine polishes the grid
argmax of a window with a deterministic, bounded compass search.  The device (refine_kernel, bmx_ctx_refine) implements
exactly the rules below; the CPU tests run compass() with a host restatement of T as objective.

Objective.  For one window (test position tg, site indices [win_lo, win_hi]) at an arbitrary point (A, x, alpha_beta):

    T = 2 * sum_i log1p(alpha_i * R_i)     over the sites i with A * |g_i - tg| <= zcut and g_i != tg
    alpha_i = exp(-A * |g_i - tg|),  R_i = psel(k_i, n_i | x, alpha_beta) * prop(n_i) / g(k_i, n_i) - 1

psel is the normalised, folded beta-binomial of the statistic in use, as the selection table holds it at grid points
(reference calcBaller, BalLeRMix+_v1.py:436-507).  A window without such a site has T = -inf; a non-finite T counts as -inf.

Coordinates and bounds.  u = ln A, x, v = ln alpha_beta.  A coordinate is free when the model's grid has two or more
distinct values of it (--fixX, --fixAlpha and a one-value --listA keep it fixed exactly).  Bounds: min and max of the
transformed grid.  A point's natural value of a coordinate is the start's own grid value while the coordinate equals the
start's, else x itself, exp(u) or exp(v).

Start: the scan's argmax.  Initial step of a free coordinate: half the smaller of the gaps between the start value and its
neighbours in the sorted transformed grid (the one gap at a hull end).

Round: candidates c -/+ h_j e_j in the order u-, u+, x-, x+, v-, v+, each clamped to the bounds; one that clamps onto the
centre is skipped.  If the best candidate's T is strictly greater than the centre's, move there (the first in order wins
ties) and keep the steps; otherwise halve every step.  Stop when every free step is below its tolerance (TOL) or after
MAX_ROUNDS rounds.  T at the start is evaluated by the search itself.

Result: the final point, T there and nSites at its A -- only if that T is strictly greater than the scan's CLR; otherwise
the scan's row unchanged.  So the refined CLR is >= the grid CLR bit for bit.  Windows without a grid result, or whose
CLR is below --refineMin, are not refined.  A local polish of the grid argmax, not a global optimiser.
"""
import math

import numpy as np

TOL = (1e-4, 1e-5, 1e-4)          # u = ln A, x, v = ln alpha_beta
MAX_ROUNDS = 256


def to_coord(k, value):
    """Natural value of coordinate k (0: A, 1: x, 2: alpha_beta) -> the search's coordinate."""
    return float(value) if k == 1 else math.log(float(value))


def to_natural(k, coord):
    return float(coord) if k == 1 else math.exp(coord)


class Axis:
    """The transformed grid of one coordinate: sorted distinct values, whether it is free, its hull."""

    def __init__(self, k, grid):
        self.k = k
        self.values = sorted(set(to_coord(k, v) for v in grid))
        self.free = len(self.values) >= 2
        self.lo, self.hi = self.values[0], self.values[-1]

    def step0(self, coord):
        """Initial step at the grid coordinate `coord`: half the smaller neighbouring gap (0 for a fixed coordinate)."""
        if not self.free:
            return 0.0
        S = self.values
        p = S.index(coord)
        gaps = []
        if p > 0:
            gaps.append(S[p] - S[p - 1])
        if p + 1 < len(S):
            gaps.append(S[p + 1] - S[p])
        return 0.5 * min(gaps)


class Setup:
    """Bounds, free coordinates and starts of the model's grid (As, xs, abetas in any order)."""

    def __init__(self, As, xs, abetas):
        self.axes = (Axis(0, As), Axis(1, xs), Axis(2, abetas))
        self.free = tuple(a.free for a in self.axes)
        self.lo = tuple(a.lo for a in self.axes)
        self.hi = tuple(a.hi for a in self.axes)

    def start(self, A, x, abeta):
        """(coordinates, natural values, initial steps) of a start at the grid point (A, x, abeta)."""
        nat = (float(A), float(x), float(abeta))
        c = tuple(to_coord(k, v) for k, v in enumerate(nat))
        return c, nat, tuple(a.step0(c[k]) for k, a in enumerate(self.axes))


def natural_of(c, c0, nat0):
    """Natural values of the point c of a search that started at c0 (whose natural values are nat0)."""
    return tuple(nat0[k] if c[k] == c0[k] else to_natural(k, c[k]) for k in range(3))


def _finite(v):
    v = float(v)
    return v if math.isfinite(v) else -math.inf


def compass(f, start, free, lo, hi, h0, tol=TOL, max_rounds=MAX_ROUNDS):
    """The compass search of the module docstring on the objective f(coordinates) -> T.
    Returns (coordinates, T, rounds, final steps)."""
    c = tuple(float(v) for v in start)
    h = [float(v) for v in h0]
    Tc = _finite(f(c))
    rounds = 0
    while rounds < max_rounds and not all(h[k] < tol[k] for k in range(3) if free[k]):
        best, move = Tc, None
        for d in range(6):
            k = d // 2
            if not free[k]:
                continue
            v = min(max(c[k] + h[k] if d & 1 else c[k] - h[k], lo[k]), hi[k])
            if v == c[k]:
                continue
            cand = c[:k] + (v,) + c[k + 1:]
            T = _finite(f(cand))
            if T > best:
                best, move = T, cand
        if move is not None:
            c, Tc = move, best
        else:
            h = [v * 0.5 for v in h]
        rounds += 1
    return c, Tc, rounds, tuple(h)


def coord_objective(T_natural, c0, nat0):
    """f(coordinates) for compass() from T_natural(A, x, abeta), with the start's natural values as the device keeps them."""
    return lambda c: T_natural(*natural_of(c, c0, nat0))


def refine_window(T_natural, setup, A, x, abeta, grid_clr):
    """One window from its grid argmax: (clr, A, x, abeta, rounds, improved) -- the scan's values where not improved."""
    c0, nat0, h0 = setup.start(A, x, abeta)
    c, T, rounds, _ = compass(coord_objective(T_natural, c0, nat0), c0, setup.free, setup.lo, setup.hi, h0)
    if T > grid_clr:
        return (T,) + natural_of(c, c0, nat0) + (rounds, True)
    return (grid_clr, float(A), float(x), float(abeta), rounds, False)


# ---------------------------------------------------------------------------------------------------------- output

def output_name(outfile):
    return outfile + '.refined.txt'


def improved_rows(clr, rclr):
    """Test sites whose refined CLR is strictly greater than the scan's."""
    return np.nonzero(np.asarray(rclr, dtype=np.float64) > np.asarray(clr, dtype=np.float64))[0]


def write_refined(path, main_path, ts, clr, refined):
    """<out>.refined.txt: the main output's lines with columns CLR, x_hat, s_hat, A_hat and nSites of the improved rows
    replaced by repr of the refined values.  refined: (clr, A, x, abeta, nsites) arrays of the test sites (fetch_refined);
    every other line, header and NA rows included, is the main output's own."""
    with open(main_path) as f:
        lines = f.readlines()
    rclr, rA, rx, rab, rns = refined
    order = ts.order if ts.na_rows else None
    for j in improved_rows(clr, rclr).tolist():
        pos = 1 + (order[j] if order is not None else j)
        head = lines[pos].rstrip('\n').split('\t')[:2]
        lines[pos] = '\t'.join(head + [repr(float(rclr[j])), repr(float(rx[j])), repr(float(rab[j])), repr(float(rA[j])),
                                       repr(int(rns[j]))]) + '\n'
    with open(path, 'w') as f:
        f.writelines(lines)


def refine_and_write(ctx, outfile, ts, min_clr):
    """After the observed scan of one file on ctx's selected slot: refine it and write <outfile>.refined.txt."""
    if len(ts) == 0:
        with open(outfile) as f, open(output_name(outfile), 'w') as g:
            g.write(f.read())
        return
    clr = ctx.fetch()[0]
    ctx.refine(min_clr)
    r = ctx.fetch_refined()
    write_refined(output_name(outfile), outfile, ts, clr, (r['clr'], r['A'], r['x'], r['abeta'], r['nsites']))
