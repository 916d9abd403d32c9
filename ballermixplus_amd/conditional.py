"""Conditional CLRs of neighbouring peaks: the definition behind --conditional, a plain host restatement, the rule that names
each apex's parent, and the writers.

What it answers.  --peaks G separates loci by G alone, and a strong locus lifts the CLR of every test site around it.  For two
nearby apexes --conditional asks: is the second still there once the first is accounted for?

A pair.  A candidate window -- test site t of the slot: position tg, site indices [win_lo[t], win_hi[t]] -- and a conditioning
locus: test site c of the same slot (position tc, its own window bounds) held at ONE grid point lin_c = (iA_c * nx + ix_c) * nab +
ia_c, i.e. (A_c, x_c, abeta_c).  For site i with table row r_i:

    candidate side, exactly the surfaces' rule (surfaces.py):
        z_i = A * |g_i - tg|;  the site is in the sum iff it lies in the clipped window, z_i <= zcut and g_i != tg
        alpha_i = exp(-z_i),  R_i = R[ix][ia][r_i]
    conditioning side: the site is SHARED iff
        max(win_lo[c], 0) <= i <= min(win_hi[c], N - 1),  zc_i = A_c * |g_i - tc| <= zcut (that single product),  g_i != tc
        shared: d_i = exp(-zc_i) * R[ix_c][ia_c][r_i];   any other site: d_i = 0.0 exactly

The model under the candidate is a nested mixture: with probability alpha_i the site is linked to the candidate, otherwise it
follows the fitted conditioning model g (1 + d_i).  The weights alpha, (1 - alpha) alpha_c and (1 - alpha)(1 - alpha_c) are always a
proper distribution, so nothing is clamped.  The log ratio against the conditioning model alone is

    T_cond(A, x, abeta) = 2 * sum_i log1p(u_i * (R_i - d_i)),    u_i = alpha_i / (1.0 + d_i)

over the candidate's sites in increasing site index; NaN where no site qualifies at that A.  nsites[iA] is the surfaces' count,
nshared[iA] the number of those sites that are shared.  Non-finite terms propagate as they do in surfaces.host_surface.  With
c < 0 or lin_c < 0 (no conditioning locus) every d_i is 0.

Two consequences the tests lean on.
  1. With every d_i == 0.0 -- no conditioning locus, or one out of reach of every site of the window -- u_i == alpha_i and
     R_i - 0.0 == R_i: T_cond is BITWISE bmx_ctx_surfaces' T of that window and nshared is 0, with or without FMA contraction.
  2. T_cond(pair) + 2 sum_i log1p(d_i) over the candidate's sites is the log ratio of the three-way mixture against neutrality.

The device (cond_surfaces_kernel, bmx_ctx_cond_surfaces) computes the surfaces of a list of pairs in one launch and each pair's
maximum by the scan's rule (influence.scan_argmax); host_cond_surface() below is the numpy restatement.

Parents (parents()).  For apex j the candidates are the apexes q != j with clr_q > clr_j -- or the same CLR and an earlier row --
and |g_q - g_j| <= H, where H = --condSpan if given, else zcut / A_hat_q + zcut / A_hat_j: the two fitted footprints can share a
site.  The parent is the candidate with the highest CLR, the earlier row on a tie; -1 without a candidate.  All comparisons are
exact FP64.

The CLI (--conditional [--condSpan H] [--condMin C] [--condSurfaces], needs --peaks).  After the peak call of the observed scan
one call carries, per kept apex j (CLR >= C; parents are chosen among ALL apexes) with parent q, the pairs (j | none),
(j | q at its scan argmax), (q | j at its scan argmax), (q | none); an apex without a parent carries (j | none) only.

Output.  <out>.conditional.txt, tab-separated, floats as repr, one row per kept apex in position order: physPos genPos CLR (the
main output's strings), T_max (the unconditional maximum of the plain-sum surface), parent_physPos parent_genPos parent_CLR,
nShared (at the apex's own scan-argmax A), CLR_cond x_cond s_cond A_cond nSites_cond (the conditional maximum and where it sits,
as the main output prints grid values; 0.0 and NA when nothing is > 0), retained = CLR_cond / T_max (like against like: both are
plain sums), parent_CLR_cond and parent_retained (the same for the parent given this apex).  Everything from parent_physPos on is
NA for an apex without a parent; a file without peaks gets the header only.  With --condSurfaces
<out>.conditional.surfaces.txt: the (j | parent) surfaces in the surfaces' format.

What this is not.  It conditions on ONE locus held at its GRID argmax: the parent is not refitted, jointly or otherwise.  The
nested mixture is asymmetric: (j | q) and (q | j) are different models, not two views of one.  Sites are linked, so `retained`
describes and does not test.  It covers the observed scan only.
"""
import numpy as np

from . import influence, surfaces

HEADER = ('physPos\tgenPos\tCLR\tT_max\tparent_physPos\tparent_genPos\tparent_CLR\tnShared\tCLR_cond\tx_cond\ts_cond\tA_cond\t'
          'nSites_cond\tretained\tparent_CLR_cond\tparent_retained\n')
HOST_BYTES = surfaces.HOST_BYTES


def value_refusal(span, min_clr):
    """The message that refuses these values of --condSpan / --condMin, or None."""
    if span is not None and not span > 0:
        return '--condSpan takes a distance > 0 in the units of the test positions.'
    if min_clr is not None and min_clr != min_clr:
        return '--condMin takes a number.'
    return None


# ----------------------------------------------------------------------------------------------- the host restatement

def host_cond_surface(genpos, rows, R, A, tg, lo, hi, tc, clo, chi, A_c, ix_c, ia_c, zcut, scale=False):
    """The conditional surface of one pair in numpy: d and `shared` of the window's sites by the definition above, then
    surfaces.host_sided_surface, the body shared with stepwise.host_base_surface.  genpos[N], rows[N], R[nx][nab][table
    rows], A: the grid in the order wanted; (tg, lo, hi): the candidate window; (tc, clo, chi): the conditioning locus' position
    and inclusive site index window, held at (A_c, ix_c, ia_c) -- tc None: no conditioning locus; zcut: bmx_alpha_cut().
    Returns (T[nA][nx][nab], NaN where no site qualifies; nsites[nA]; nshared[nA]) and with scale=True also S[nA][nx][nab] =
    2 sum_i |term_i| (0 where no site qualifies): the size of what cancels in T."""
    def side(a, b, gw, rw, R):
        d, shared = np.zeros(len(gw)), np.zeros(len(gw), dtype=bool)
        if tc is not None:
            idx = np.arange(a, b + 1, dtype=np.int64)
            zc = A_c * np.abs(gw - tc)
            shared = (idx >= max(int(clo), 0)) & (idx <= min(int(chi), len(genpos) - 1)) & (zc <= zcut) & (gw != tc)
            with np.errstate(over='ignore', invalid='ignore'):
                d[shared] = np.exp(-zc[shared]) * R[int(ix_c), int(ia_c), rw[shared]]
        return d, shared

    return surfaces.host_sided_surface(genpos, rows, R, A, tg, lo, hi, side, zcut, scale)


def parents(gen, clr, iA_hat, grid_A, apex_rows, zcut, span=None):
    """The parent of every apex by the rule of the definition.  gen[M], clr[M], iA_hat[M]: the track's test positions, CLR and the
    scan argmax's index into grid_A (scan order); apex_rows: the rows of the peak call; span: H, or None for the sum of the two
    fitted reaches.  Returns int64[K]: for apex k the place IN apex_rows of its parent, -1 without one."""
    rows = np.asarray(apex_rows, dtype=np.int64)
    g, c = np.asarray(gen, dtype=np.float64)[rows], np.asarray(clr, dtype=np.float64)[rows]
    iA = np.asarray(iA_hat, dtype=np.int64)[rows]
    with np.errstate(divide='ignore'):
        reach = np.where(iA >= 0, zcut / np.asarray(grid_A, dtype=np.float64)[np.maximum(iA, 0)], 0.0)      # no grid result: no footprint
    out = np.full(len(rows), -1, dtype=np.int64)
    for j in range(len(rows)):
        best = -1
        for q in range(len(rows)):
            if q == j or not (c[q] > c[j] or (c[q] == c[j] and rows[q] < rows[j])):
                continue
            H = float(span) if span is not None else reach[q] + reach[j]
            if not abs(g[q] - g[j]) <= H:
                continue
            if best < 0 or c[q] > c[best] or (c[q] == c[best] and rows[q] < rows[best]):
                best = q
        out[j] = best
    return out


def pair_list(apex_rows, parent, lin, keep=None):
    """The pairs of one call.  apex_rows[K], parent[K] (parents()), lin[M]: the scan argmax of every track row, keep: the places
    in apex_rows that get a row (None: all).  Returns (tests, cond_test, cond_lin: int32 lists for Context.cond_surfaces; where:
    per kept apex its place k and the entries (k | none), (k | q), (q | k), (q | none) in the lists, the last three -1 without
    a parent)."""
    rows = np.asarray(apex_rows, dtype=np.int64)
    lin = np.asarray(lin)
    tests, ctest, clin, where = [], [], [], []
    for k in (range(len(rows)) if keep is None else keep):
        j, q = int(rows[k]), int(parent[k])
        at = len(tests)
        tests.append(j); ctest.append(-1); clin.append(-1)
        if q < 0:
            where.append((int(k), at, -1, -1, -1))
            continue
        p = int(rows[q])
        tests += [j, p, p]
        ctest += [p, j, -1]
        clin += [int(lin[p]), int(lin[j]), -1]
        where.append((int(k), at, at + 1, at + 2, at + 3))
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    return i32(tests), i32(ctest), i32(clin), where


# ---------------------------------------------------------------------------------------------------------- output

def output_name(outfile):
    return outfile + '.conditional.txt'


def surfaces_name(outfile):
    return outfile + '.conditional.surfaces.txt'


_num = influence._num
read_table = influence.read_table


def _ratio(a, b):
    return float(a) / float(b) if b > 0 else None


def table_rows(phys, gen, clr, apex_rows, parent, iA_hat, where, res, sel):
    """The rows of <out>.conditional.txt.  phys, gen, clr: the main output's strings of EVERY apex (in apex_rows' order);
    iA_hat[M]: the scan argmax's A index of every track row; (where, res): pair_list()'s places and Context.cond_surfaces' dict of
    the same call; sel: the run's NormalizedBetaBinom (the grids in scan order)."""
    npairs = len(sel.grid_x) * len(sel.grid_abeta)
    out = []
    for k, none, cond, pcond, pnone in where:
        T_max = float(res['tmax'][none])
        head = [phys[k], gen[k], clr[k], repr(T_max)]
        if cond < 0:
            out.append('\t'.join(head + ['NA'] * 12) + '\n')
            continue
        q = int(parent[k])
        l = int(res['lin'][cond])
        v = float(res['tmax'][cond])
        own_iA = int(iA_hat[int(apex_rows[k])])
        cols = [phys[q], gen[q], clr[q], _num(int(res['nshared'][cond][own_iA]) if own_iA >= 0 else None), repr(v)]
        cols += list(influence.grid_strings(l, sel)) + [_num(int(res['nsites'][cond][l // npairs]) if l >= 0 else None)]
        pv = float(res['tmax'][pcond])
        cols += [_num(_ratio(v, T_max)), repr(pv), _num(_ratio(pv, float(res['tmax'][pnone])))]
        out.append('\t'.join(head + cols) + '\n')
    return out


def write_table(path, rows):
    with open(path, 'w') as f:
        f.write(HEADER)
        f.writelines(rows)


def conditional_and_write(ctx, outfile, ts, sel, apex_rows, span=None, min_clr=None, with_surfaces=False, host_bytes=HOST_BYTES):
    """After the observed scan of one file on ctx's selected slot and its peak call (apex_rows): name the parents, compute the
    pairs in one call and write <outfile>.conditional.txt (with_surfaces: also <outfile>.conditional.surfaces.txt, the (j |
    parent) surfaces fetched in batches of at most host_bytes).  sel: the run's NormalizedBetaBinom (the grids in scan order).
    Returns (rows written, how many of them have a parent)."""
    apex = np.asarray(apex_rows, dtype=np.int64)
    rows, where, parent = [], [], np.zeros(0, dtype=np.int64)
    if len(ts) and len(apex):
        nx, nab = len(sel.grid_x), len(sel.grid_abeta)
        clr, ix, ia, iA, _ = ctx.fetch()
        lin = np.where(iA >= 0, (iA.astype(np.int64) * nx + ix) * nab + ia, -1)
        zcut = float(ctx._L.bmx_alpha_cut())
        grid_A = np.array([float(v) for v in sel.grid_A])
        parent = parents(ts.test_gen, clr, iA, grid_A, apex, zcut, span)
        keep = [k for k in range(len(apex)) if min_clr is None or clr[apex[k]] >= min_clr]
        tests, ctest, clin, where = pair_list(apex, parent, lin, keep)
        res = ctx.cond_surfaces(tests, ctest, clin, want_T=False)
        phys, gen = surfaces.labels(ts, apex.tolist())
        rows = table_rows(phys, gen, [repr(float(v)) for v in clr[apex]], apex, parent, iA, where, res, sel)
    write_table(output_name(outfile), rows)
    with_parent = [w for w in where if w[2] >= 0]
    if with_surfaces:
        layout = surfaces.Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)
        batch = max(1, int(host_bytes) // (8 * max(layout.points, 1)))
        with open(surfaces_name(outfile), 'w') as f:
            f.write(surfaces.HEADER)
            for b in range(0, len(with_parent), batch):
                part = with_parent[b:b + batch]
                at = [w[2] for w in part]
                r = ctx.cond_surfaces(tests[at], ctest[at], clin[at])
                surfaces.write_blocks(f, layout, [phys[w[0]] for w in part], [gen[w[0]] for w in part], r['T'], r['nsites'])
    return len(rows), len(with_parent)
