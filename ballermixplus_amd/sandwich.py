"""Sandwich (Godambe) standard errors of a window's fitted point: the definition behind --sandwich, a plain host restatement, the
per-window summary, and the writer.

What it answers.  T is a composite likelihood: it multiplies the sites' marginal likelihoods as if the sites were independent.
Its curvature H alone therefore overstates how well x, alpha_beta and A are determined.  The textbook repair is the sandwich
variance V = H^-1 J H^-1, with H the sensitivity and J the variability of the composite score, estimated from the sums of the
per-site scores over blocks of consecutive sites.  It costs one pass over the window's sites at one point, and it yields the
first-order scale lambda = tr(H^-1 J) / p by which linkage inflates the CLR.

Coordinates and sites.  theta = (u, x, v) = (ln A, x, ln alpha_beta), the refinement's coordinates (refine.py).  For one window
(test position tg, site indices [win_lo, win_hi], clipped to the chromosome) at a caller-given point (A, x, alpha_beta) the sites
are the surfaces' sites: z_i = A * |g_i - tg| <= zcut (that single product) and g_i != tg.  Per site alpha_i = exp(-z_i),
R_i = R(row_i | x, alpha_beta) -- the off-grid table entry of the refinement (refine_R on the device, Context.refine_R) -- and
D_i = 1 + alpha_i R_i.

Table derivatives.  Central differences with the steps hx, hv (defaults HX, HV):
    Rx_i = (R(row_i | x + hx, alpha_beta) - R(row_i | x - hx, alpha_beta)) / (2 hx)
    Rv_i = (R(row_i | x, alpha_beta * rv) - R(row_i | x, alpha_beta / rv)) / (2 hv),    rv = exp(hv)
rv is computed once on the host by the C library's exp (math.exp gives the same double); x - hx and x + hx are the plain IEEE
sums: shifted_points() below returns the five (x, alpha_beta) exactly as the library forms them.

Site score and T.  s_i = (-z_i alpha_i R_i / D_i, alpha_i Rx_i / D_i, alpha_i Rv_i / D_i).  The u-component is analytic
(d alpha / du = -z alpha); the dependence of the window's membership on A is ignored: a site at the cut has alpha = 1e-8.  A site
whose D_i is not > 0, or whose score is not finite, is SKIPPED: it is counted in nSites and in nSkipped and enters no sum (--fit's
rule for such sites).  T = 2 * sum log1p(alpha_i R_i) over the used sites, -inf without one.

g, H, J and blocks.  g = sum_i s_i (about 0 at an interior maximum: a diagnostic).  H = sum_i s_i s_i^T: the sensitivity by the
second Bartlett identity, which every site's marginal model satisfies, so no second derivative is needed.  The block of site i is
i // B in the slot's site array (--boot's and --influence's rule); S_b = the sum of s_i over the block's used sites in this window;
J = sum_b S_b S_b^T; nBlocks = the blocks with a used site.  A symmetric matrix travels as six doubles (uu, ux, uv, xx, xv, vv).
Two identities follow: with B = 1, J is H; if every site stands m times at one position and B = m with aligned blocks, J = m H.

Device (sandwich_kernel, bmx_ctx_sandwich; include/bmxscan.h).  One workgroup per listed window, no atomics, every sum in a fixed
order; with B = 1 J equals H bit for bit.  host_sandwich() below is the per-window numpy restatement the tests compare it with:
the counts exactly, T to 1e-12 relative, g, H and J within 1e-12 of the sum of their absolute terms, when it is fed the device's own
five columns.

Summary (summarise()).  The KEPT coordinates are those the model's grid leaves free (refine.Setup.free) whose value at the point
lies strictly inside the grid's hull (by more than HULL_EPS, relative: a refined point clamped to the hull comes back through
exp).  A free coordinate on the hull is constrained, its score is not zero; it is named in the column on_hull and dropped.  (With
the default grid x = 0.5 is on the hull; there Rx = 0 by the table's symmetry in x <-> 1 - x, so dropping it also keeps H
regular.)  On the p kept coordinates:
    V = H^-1 J H^-1,  se = sqrt(diag V),  se_naive = sqrt(diag H^-1) (what one gets treating the sites as independent),
    lambda_mean = tr(H^-1 J) / p,  lambda_max = the largest eigenvalue of H^-1 J,  CLR_adj = T / lambda_mean,
    grad_norm = sqrt(g^T H^-1 g).
Status: `singular` when p = 0 or H scaled to unit diagonal has a reciprocal condition number below RCOND_MIN = 1e-10 (everything
after nBlocks is then NA); `unstable` when the standard errors move by more than FD_REL_MAX = 0.1, relative, between the steps
(hx, hv) and (2 hx, 2 hv) (fd_rel: the largest such change of a kept coordinate; the first call's numbers are still printed);
`ok` otherwise.

The default steps HX = 1e-3, HV = 1e-2 were measured on the host with a scipy-made table (n = 100, B_2, min count 1,
x in {0.1, 0.3, 0.45}; tests/test_sandwich_cpu.py repeats it): the information-weighted error of the central difference against the
same difference at half the step is at most 3.5e-4 for alpha_beta <= 1e3.  For alpha_beta >= 1e6 it is O(1): ln alpha_beta
carries no information there (about 1e-9 per site) and the table's rounding noise decides the difference; no step repairs
that, hence `unstable`.

What this is not.  H by the outer product assumes each site's marginal model.  Blocks are independent only beyond B sites.  The
number of effective blocks is small, because alpha concentrates the weight near the test site.  The null alpha = 0 lies on the
boundary of the parameter space, so CLR_adj describes and does not test.  The point is taken as given and not re-optimised (with
--refine the refined point, otherwise the grid argmax, whose score is not zero).  alpha_beta >= 1e6 is not identifiable.

Selection.  As --surfaces selects (surfaces.select): --sandwichMin C, with --peaks only the apexes, at most --sandwichMax N.

Output.  <out>.sandwich.txt, tab-separated, floats as repr, one row per selected window in the main output's order: HEADER below.
physPos genPos CLR are the main output's strings; x_hat s_hat A_hat the point used.  point is `refined` where the window was
refined (rounds >= 0), else `grid`; a refined window whose search did not improve on the scan keeps the grid point, and its
x_hat s_hat A_hat are then the main output's strings, as <out>.refined.txt prints such a row.  The se columns of a fixed or on-hull
coordinate are NA.
"""
import math

import numpy as np

from . import influence, refine, surfaces

HX, HV = 1e-3, 1e-2
RCOND_MIN = 1e-10
FD_REL_MAX = 0.1
HULL_EPS = 1e-12
MAX_WINDOWS = surfaces.MAX_WINDOWS
HOST_WINDOWS = 1 << 16          # the writer asks for at most this many windows at a time
NAMES = ('lnA', 'x', 'lns')     # the coordinates u, x, v in the output's words
ORDER = (1, 2, 0)               # column order of the coordinates: x, s (alpha_beta), A
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # the six travelling entries

HEADER = ('physPos\tgenPos\tCLR\tx_hat\ts_hat\tA_hat\tnSites\tnSkipped\tnBlocks\tpoint\ton_hull\tx_se\tlns_se\tlnA_se\t'
          'x_se_naive\tlns_se_naive\tlnA_se_naive\tlambda_mean\tlambda_max\tCLR_adj\tgrad_norm\tfd_rel\tstatus\n')


def value_refusal(block, min_clr, max_n, step):
    """The message that refuses these values of --sandwichBlock / --sandwichMin / --sandwichMax / --sandwichStep (None: the flag
    was not given), or None."""
    if block is not None and block < 1:
        return '--sandwichBlock takes a number of sites >= 1.'
    if min_clr is not None and min_clr != min_clr:
        return '--sandwichMin takes a number.'
    if max_n is not None and max_n < 1:
        return '--sandwichMax takes a number of windows >= 1.'
    if step is not None:
        try:
            parse_step(step)
        except ValueError as e:
            return str(e)
    return None


def parse_step(text):
    """'hx,hv' -> (hx, hv), both finite and > 0."""
    parts = str(text).split(',')
    try:
        hx, hv = (float(p) for p in parts)
    except ValueError:
        raise ValueError('--sandwichStep takes two numbers hx,hv (the steps in x and in ln alpha_beta).')
    if not (math.isfinite(hx) and hx > 0.0 and math.isfinite(hv) and hv > 0.0):
        raise ValueError('--sandwichStep takes two finite steps > 0.')
    return hx, hv


def shifted_points(x, abeta, hx=HX, hv=HV):
    """The five (x, alpha_beta) of the table columns, as the library forms them: the point, x - hx, x + hx, alpha_beta / rv,
    alpha_beta * rv with rv = math.exp(hv)."""
    x, abeta = float(x), float(abeta)
    rv = math.exp(float(hv))
    return ((x, abeta), (x - float(hx), abeta), (x + float(hx), abeta), (x, abeta / rv), (x, abeta * rv))


def sym3(v):
    """Six travelling entries -> the 3 x 3 symmetric matrix."""
    M = np.zeros((3, 3))
    for e, (k, l) in enumerate(SYM):
        M[k, l] = M[l, k] = float(v[e])
    return M


# ----------------------------------------------------------------------------------------------- the host restatement

def site_scores(genpos, rows, tabs, A, tg, lo, hi, hx, hv, zcut):
    """The per-site quantities of one window: (site indices of its sites, s[n][3], log1p(alpha R)[n], used bool[n])."""
    g = np.asarray(genpos, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    tabs = np.asarray(tabs, dtype=np.float64)
    a, b = max(int(lo), 0), min(int(hi), len(g) - 1)
    if b < a:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0), np.zeros(0, dtype=bool)
    gw_ = g[a:b + 1]
    z = float(A) * np.abs(gw_ - tg)
    keep = (z <= zcut) & (gw_ != tg)
    idx = a + np.nonzero(keep)[0].astype(np.int64)
    z = z[keep]
    r = rows[idx]
    alpha = np.exp(-z)
    with np.errstate(all='ignore'):
        R0 = tabs[0][r]
        Rx = (tabs[2][r] - tabs[1][r]) / (2.0 * float(hx))
        Rv = (tabs[4][r] - tabs[3][r]) / (2.0 * float(hv))
        aR = alpha * R0
        D = 1.0 + aR
        s = np.stack([-z * aR / D, alpha * Rx / D, alpha * Rv / D], axis=1) if len(idx) else np.zeros((0, 3))
        lt = np.log1p(aR)
        used = (D > 0.0) & np.all(np.isfinite(s), axis=1)
    return idx, s, lt, used


def host_sandwich(genpos, rows, tabs, A, tg, lo, hi, block=1, hx=HX, hv=HV, zcut=None):
    """The pieces of one window in numpy.  genpos[N], rows[N]: position and table row of every site; tabs[5][table rows]: the
    columns R at shifted_points(); A: the point's A; (tg, lo, hi): the window; zcut: bmx_alpha_cut().  Returns a dict: T, g[3],
    H[6], J[6], nsites, nskipped, nblocks, and absg[3], absH[6], absJ[6]: the sums of the absolute terms (for J entry (k, l)
    sum_b (sum_i |s_ik|)(sum_i |s_il|)), the scale of the tests' tolerance."""
    if zcut is None:
        from . import power
        zcut = power.ALPHA_CUT
    idx, s, lt, used = site_scores(genpos, rows, tabs, A, tg, lo, hi, hx, hv, zcut)
    out = {'nsites': int(len(idx)), 'nskipped': int(np.count_nonzero(~used))}
    idx, s, lt = idx[used], s[used], lt[used]
    out['T'] = 2.0 * float(np.sum(lt)) if len(idx) else -math.inf
    out['absT'] = 2.0 * float(np.sum(np.abs(lt)))
    blk = idx // int(block)
    ub, inv = np.unique(blk, return_inverse=True)
    S, Sabs = np.zeros((len(ub), 3)), np.zeros((len(ub), 3))
    np.add.at(S, inv, s)
    np.add.at(Sabs, inv, np.abs(s))
    out['nblocks'] = int(len(ub))
    out['g'] = s.sum(axis=0) if len(idx) else np.zeros(3)
    out['absg'] = np.abs(s).sum(axis=0) if len(idx) else np.zeros(3)
    out['H'] = np.array([np.sum(s[:, k] * s[:, l]) for k, l in SYM])
    out['absH'] = np.array([np.sum(np.abs(s[:, k] * s[:, l])) for k, l in SYM])
    out['J'] = np.array([np.sum(S[:, k] * S[:, l]) for k, l in SYM])
    out['absJ'] = np.array([np.sum(Sabs[:, k] * Sabs[:, l]) for k, l in SYM])
    return out


# ------------------------------------------------------------------------------------------------------------ summary

def kept_coordinates(setup, point):
    """(kept, on_hull): the coordinate numbers (0: u, 1: x, 2: v) of the definition at point = (A, x, alpha_beta)."""
    kept, hull = [], []
    for k in range(3):
        if not setup.free[k]:
            continue
        c = refine.to_coord(k, point[k])
        lo, hi = setup.lo[k], setup.hi[k]
        eps = HULL_EPS * max(1.0, abs(lo), abs(hi))
        (kept if lo + eps < c < hi - eps else hull).append(k)
    return tuple(kept), tuple(hull)


def summarise(T, g, H, J, setup, point):
    """The per-window numbers of the definition from one window's pieces: a dict with kept, on_hull (coordinate numbers), status
    ('ok' or 'singular') and -- None where the definition says NA -- se[3], se_naive[3] (None for a coordinate not kept),
    lambda_mean, lambda_max, CLR_adj, grad_norm; with status 'ok' also eigenvalues: those of H^-1 J, ascending."""
    kept, hull = kept_coordinates(setup, point)
    out = {'kept': kept, 'on_hull': hull, 'status': 'singular', 'se': [None] * 3, 'se_naive': [None] * 3, 'lambda_mean': None,
           'lambda_max': None, 'CLR_adj': None, 'grad_norm': None}
    p = len(kept)
    if p == 0:
        return out
    at = np.ix_(kept, kept)
    Hk, Jk, gk = sym3(H)[at], sym3(J)[at], np.asarray(g, dtype=np.float64)[list(kept)]
    d = np.sqrt(np.diag(Hk))
    if not (np.all(np.isfinite(Hk)) and np.all(np.isfinite(Jk)) and np.all(np.isfinite(gk)) and np.all(d > 0.0)):
        return out
    Hs = Hk / np.outer(d, d)
    sv = np.linalg.svd(Hs, compute_uv=False)
    if not (sv[0] > 0.0 and sv[-1] / sv[0] >= RCOND_MIN):
        return out
    Hinv = np.linalg.inv(Hs) / np.outer(d, d)
    V = Hinv @ Jk @ Hinv
    M = Hinv @ Jk
    L = np.linalg.cholesky(Hs)                                   # H^-1 J is similar to the symmetric L^-1 Js L^-T
    W = np.linalg.solve(L, np.linalg.solve(L, Jk / np.outer(d, d)).T)
    lam = np.linalg.eigvalsh(0.5 * (W + W.T))
    out['status'] = 'ok'
    for j, k in enumerate(kept):
        out['se'][k] = math.sqrt(max(float(V[j, j]), 0.0))
        out['se_naive'][k] = math.sqrt(max(float(Hinv[j, j]), 0.0))
    out['lambda_mean'] = float(np.trace(M)) / p
    out['lambda_max'] = float(lam[-1])
    out['eigenvalues'] = lam
    if out['lambda_mean'] > 0.0 and math.isfinite(float(T)):
        out['CLR_adj'] = float(T) / out['lambda_mean']
    out['grad_norm'] = math.sqrt(max(float(gk @ Hinv @ gk), 0.0))
    return out


def fd_rel(first, second):
    """The largest relative change of a kept coordinate's se between the summaries of the two calls (steps (hx, hv) and
    (2 hx, 2 hv)); None when the first is singular, inf when only the second is."""
    if first['status'] == 'singular':
        return None
    if second['status'] == 'singular':
        return math.inf
    worst = 0.0
    for k in first['kept']:
        a, b = first['se'][k], second['se'][k]
        worst = max(worst, abs(b - a) / a if a > 0.0 else (0.0 if b == a else math.inf))
    return worst


def status_of(first, rel):
    """`singular`, `unstable` (fd_rel > FD_REL_MAX) or `ok`."""
    if first['status'] == 'singular':
        return 'singular'
    return 'unstable' if rel is not None and rel > FD_REL_MAX else 'ok'


# ---------------------------------------------------------------------------------------------------------- output

def output_name(outfile):
    return outfile + '.sandwich.txt'


_num = influence._num
read_table = influence.read_table


def summary_row(phys, gen, clr, point_strings, counts, which, first, rel):
    """One row of <out>.sandwich.txt: (phys, gen, clr) the main output's strings, point_strings = (x_hat, s_hat, A_hat), counts =
    (nSites, nSkipped, nBlocks), which = 'refined' or 'grid', first = summarise() of the first call, rel = fd_rel()."""
    cols = [phys, gen, clr] + list(point_strings) + [str(int(v)) for v in counts]
    cols += [which, ','.join(NAMES[k] for k in ORDER if k in first['on_hull']) or '.']
    if first['status'] == 'singular':
        return '\t'.join(cols + ['NA'] * 11 + ['singular']) + '\n'
    cols += [_num(first['se'][k]) for k in ORDER] + [_num(first['se_naive'][k]) for k in ORDER]
    cols += [_num(first[k]) for k in ('lambda_mean', 'lambda_max', 'CLR_adj', 'grad_norm')]
    return '\t'.join(cols + ['inf' if rel == math.inf else _num(rel), status_of(first, rel)]) + '\n'


def rows_of(phys, gen, clr, point_strings, which, points, setup, first, second):
    """The file's rows of len(phys) windows from the two calls' dicts (Context.sandwich at (hx, hv) and at (2 hx, 2 hv)); points[n]
    = (A, x, alpha_beta) of every window."""
    out = []
    for w in range(len(phys)):
        s1 = summarise(first['T'][w], first['g'][w], first['H'][w], first['J'][w], setup, points[w])
        s2 = summarise(second['T'][w], second['g'][w], second['H'][w], second['J'][w], setup, points[w])
        counts = (first['nsites'][w], first['nskipped'][w], first['nblocks'][w])
        out.append(summary_row(phys[w], gen[w], clr[w], point_strings[w], counts, which[w], s1, fd_rel(s1, s2)))
    return out


def write_sandwich(outfile, rows):
    """The whole file from rows_of()'s rows (the tests' entry point)."""
    with open(output_name(outfile), 'w') as f:
        f.write(HEADER)
        f.writelines(rows)


def points_of(ctx, sel, refined=None):
    """Every window's point after the observed scan: (A[M], x[M], abeta[M], refined bool[M], lin[M], improved bool[M]:
    the refined CLR is above the scan's, so the point is no grid point).  refined: fetch_refined()'s
    dict (the refined point where rounds >= 0), or None: the grid argmax everywhere; NaN where the row has no grid result."""
    clr, ix, ia, iA, _ = ctx.fetch()
    ok = iA >= 0
    gA, gx, gab = (np.asarray(v, dtype=np.float64) for v in (sel.grid_A, sel.grid_x, sel.grid_abeta))
    A = np.where(ok, gA[np.maximum(iA, 0)], np.nan)
    x = np.where(ok, gx[np.maximum(ix, 0)], np.nan)
    ab = np.where(ok, gab[np.maximum(ia, 0)], np.nan)
    lin = np.where(ok, (iA.astype(np.int64) * len(gx) + ix) * len(gab) + ia, -1)
    ref = np.zeros(len(clr), dtype=bool)
    if refined is not None:
        ref = ok & (np.asarray(refined['rounds']) >= 0)
        A, x, ab = np.where(ref, refined['A'], A), np.where(ref, refined['x'], x), np.where(ref, refined['abeta'], ab)
    imp = ref & (np.asarray(refined['clr']) > clr) if refined is not None else ref
    return A, x, ab, ref, lin, imp


def sandwich_and_write(ctx, outfile, ts, sel, block=1, min_clr=0.0, max_n=MAX_WINDOWS, hx=HX, hv=HV, apex_rows=None, refined=False,
                       host_windows=HOST_WINDOWS):
    """After the observed scan of one file on ctx's selected slot (its peak call and, with refined=True, its refinement): select
    the windows as --surfaces does, compute each one's pieces at its point with the steps (hx, hv) and (2 hx, 2 hv) and write
    <outfile>.sandwich.txt.  sel: the run's NormalizedBetaBinom (the grids in scan order).  Returns (windows written, windows
    the cap dropped).  Raises ValueError, before the file is opened, when a selected point's x is within 2 hx of 0 or 1."""
    setup = refine.Setup(sel.grid_A, sel.grid_x, sel.grid_abeta)
    rows, dropped = np.zeros(0, dtype=np.int64), 0
    if len(ts):
        clr, _, _, iA, _ = ctx.fetch()
        rows, dropped = surfaces.select(clr, iA, min_clr, apex_rows, max_n)
        A, x, ab, ref, lin, imp = points_of(ctx, sel, ctx.fetch_refined() if refined else None)
        if len(rows) and not (np.all(x[rows] - 2.0 * hx > 0.0) and np.all(x[rows] + 2.0 * hx < 1.0)):         # before the file exists
            raise ValueError('--sandwichStep: a selected window\'s x_hat is within 2 hx = %r of 0 or 1; choose a smaller hx.' % (2.0 * hx))
    with open(output_name(outfile), 'w') as f:
        f.write(HEADER)
        for k in range(0, len(rows), int(host_windows)):
            part = rows[k:k + int(host_windows)]
            first = ctx.sandwich(part, A[part], x[part], ab[part], block, hx, hv)
            second = ctx.sandwich(part, A[part], x[part], ab[part], block, 2.0 * hx, 2.0 * hv)
            phys, gen = surfaces.labels(ts, part.tolist())
            strings = [(repr(float(x[t])), repr(float(ab[t])), repr(float(A[t]))) if imp[t] else influence.grid_strings(int(lin[t]), sel)
                       for t in part.tolist()]
            which = ['refined' if ref[t] else 'grid' for t in part.tolist()]
            points = [(float(A[t]), float(x[t]), float(ab[t])) for t in part.tolist()]
            f.writelines(rows_of(phys, gen, [repr(float(v)) for v in clr[part]], strings, which, points, setup, first, second))
    return len(rows), dropped
